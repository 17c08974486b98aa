"""include/vct_motion.h without a GPU: what the restatement (tests/motion_ref.py) promises, on
planes from shading_ref.planes over objects_ref.posed_union, and that the library and the binding
carry the two functions.  The measured values are DESIGN 10.19's.
"""
import os
import subprocess

import numpy as np
import pytest

import motion_inputs as MI
import motion_ref as MR
import objects_ref as OR
import temporal_inputs as TI
import temporal_ref as TR

F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vct_objects_poses_device", "vct_objects_motion_device")
# 4 x the largest difference measured on the restatement (printed by the tests below):
BOUND_TRANSLATION = 4 * 2.61e-7     # |motion4.xyz - (P - T)|, the box moved by BOX_T, all five frames
BOUND_Q64 = 4 * 7.75e-8             # float32 against float64: the previous point
BOUND_N64 = 4 * 2.92e-8             # ... and the previous normal


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _motion(name, cur, prev, w, h, with_nrm=True, planes=None):
    meshes, _ = MI.object_set(name)
    vpos, vidx, first = MI.packed(meshes)
    pl = planes or MI.cpu_planes(name, cur, w, h)
    return pl, MR.motion(pl["pos"], pl["nrm"] if with_nrm else None, pl["tri_id"], pl["bary"], MI.n_static(), first, vpos,
                         vidx, cur, prev)


def _history(w, h, prev_planes):
    """What the accumulate needs of a previous frame: CAM_A, its G-buffer, planes and lengths."""
    hl = np.where(prev_planes["pos"][..., 3] != 0, 3, 0).astype(np.uint32)
    return dict(prev_cam=TI.cam_a(), prev_pos=prev_planes["pos"], prev_nrm=prev_planes["nrm"], hist=TI.planes(3, w, h, 2),
                hist_len=hl, plane_eps=TI.plane_eps())


# ---- (a) nothing moved ----------------------------------------------------------------------------
@pytest.mark.parametrize("frame", MI.FRAMES)
def test_unmoved_set_is_the_static_record(frame):
    w, h = frame
    _, placing = MI.object_set("catalogue")
    cur = OR.pose_array(placing)
    pl, r = _motion("catalogue", cur, cur.copy(), w, h)
    valid = pl["pos"][..., 3] != 0
    assert np.array_equal(_bits(r["motion"][..., :3]), _bits(np.where(valid[..., None], pl["pos"][..., :3], F(0))))
    assert np.array_equal(_bits(r["motion"][..., 3]), _bits(valid.astype(F)))
    assert np.array_equal(_bits(r["prev_nrm"]), _bits(pl["nrm"]))
    assert r["stats"] == (int(valid.sum()), int(valid.sum()), 0, 0)
    if frame == (64, 48):
        assert (r["obj"] >= 0).sum() > 0                      # objects are in view
    kw = _history(w, h, pl)
    cur_planes = TI.planes(4, w, h, 2)
    a = TR.accumulate(pl["pos"], pl["nrm"], cur_planes, motion=r["motion"], **kw)
    b = TR.accumulate(pl["pos"], pl["nrm"], cur_planes, motion=None, **kw)
    for x, y in zip(a["out"] + [a["out_len"]], b["out"] + [b["out_len"]]):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
    assert a["stats"] == b["stats"]


# ---- (b) a translation ----------------------------------------------------------------------------------
def test_translation_gives_the_point_minus_the_offset():
    _, placing = MI.object_set("box")
    prev = OR.pose_array(placing)
    cur = OR.pose_array([MI.TRANSITIONS[1][2](placing[0])])
    worst, seen = 0.0, 0
    for w, h in MI.FRAMES:
        pl, r = _motion("box", cur, prev, w, h)
        on = r["obj"] == 0
        assert (r["cls"][on] == MR.MOVED).all()
        want = pl["pos"][..., :3].astype(np.float64) - np.array(TI.BOX_T, F).astype(np.float64)
        d = np.abs(r["motion"][..., :3].astype(np.float64) - want)[on]
        worst, seen = max(worst, float(d.max()) if d.size else 0.0), seen + int(on.sum())
        off = (r["cls"] == MR.STILL)
        assert np.array_equal(_bits(r["motion"][off][:, :3]), _bits(pl["pos"][off][:, :3]))
    print(f"translation: {seen} pixels, largest |motion4.xyz - (P - T)| = {worst:.3e}")
    assert seen >= 150 and worst < BOUND_TRANSLATION


# ---- (c) a rotation larger than acos(normal_cos) ------------------------------------------------------------
@pytest.mark.parametrize("frame", ((32, 24), (64, 48)))
def test_rotation_needs_the_previous_normal(frame):
    w, h = frame
    assert np.cos(np.radians(MI.ANGLE)) < TR.NORMAL_COS
    _, placing = MI.object_set("box")
    prev = OR.pose_array(placing)
    cur = OR.pose_array([MI.TRANSITIONS[2][2](placing[0])])
    before = MI.cpu_planes("box", prev, w, h)
    pl, r = _motion("box", cur, prev, w, h)
    side = (r["cls"] == MR.MOVED) & (np.abs(pl["nrm"][..., 1]) < 0.5)     # normal not along the axis
    assert side.sum() >= 25
    kw = _history(w, h, before)
    cur_planes = TI.planes(4, w, h, 2)
    plain = TR.accumulate(pl["pos"], pl["nrm"], cur_planes, motion=r["motion"], **kw)
    fixed = TR.accumulate(pl["pos"], r["prev_nrm"], cur_planes, motion=r["motion"], **kw)
    n_plain, n_fixed = int((plain["cls"][side] == TR.REUSED).sum()), int((fixed["cls"][side] == TR.REUSED).sum())
    print(f"rotation {w}x{h}: {int(side.sum())} side pixels, reused {n_plain} with nrm4, {n_fixed} with prev_nrm4")
    assert n_plain == 0 and n_fixed > 0
    # off the object nothing changes: the two planes are nrm4 there
    off = r["cls"] != MR.MOVED
    assert np.array_equal(_bits(r["prev_nrm"][off]), _bits(pl["nrm"][off]))
    # the rotated normal is the previous G-buffer's at the previous point: a unit vector, 40 degrees off
    c = (r["prev_nrm"][side][:, :3].astype(np.float64) * pl["nrm"][side][:, :3]).sum(-1)
    assert np.allclose(c, np.cos(np.radians(MI.ANGLE)), atol=1e-6)


# ---- (d) float32 against float64 ------------------------------------------------------------------------------
def test_restatement_against_float64():
    worst_q = worst_n = 0.0
    pixels = 0
    for name in ("catalogue", "seventy", "box"):
        meshes, placing = MI.object_set(name)
        vpos, vidx, _ = MI.packed(meshes)
        for rnd in range(MI.ROUNDS):
            prev, cur = MI.round_poses(placing, rnd)
            pl, r = _motion(name, cur, prev, 64, 48)
            mv = r["cls"] == MR.MOVED
            if not mv.any():
                continue
            o, t = r["obj"][mv], pl["tri_id"][mv].astype(np.int64) - MI.n_static()
            args = (t, pl["bary"][mv], pl["nrm"][mv], vpos, vidx, prev["m"][o], cur["m"][o])
            q32, n32, ok32 = MR.moved_terms(F, *args)
            q64, n64, ok64 = MR.moved_terms(np.float64, *args)
            assert np.array_equal(ok32, ok64)
            assert np.array_equal(_bits(q32), _bits(r["motion"][mv][:, :3]))
            worst_q = max(worst_q, float(np.abs(q32.astype(np.float64) - q64).max()))
            if ok32.any():
                worst_n = max(worst_n, float(np.abs(n32.astype(np.float64) - n64)[ok32].max()))
            pixels += int(mv.sum())
    print(f"float32 against float64 over {pixels} moved pixels: point {worst_q:.3e}, normal {worst_n:.3e}")
    assert pixels >= 5000 and worst_q < BOUND_Q64 and worst_n < BOUND_N64


# ---- (e) hostile planes -------------------------------------------------------------------------------------------
def _one_pixel(pos, nrm, k, bary, n_st, first, vpos, vidx, cur, prev):
    """The rule for one pixel, written out case by case with scalar float32 operations."""
    from spec_ref import fmaf
    zero = np.zeros(4, F)
    if pos[3] == 0:
        return zero, zero, None
    n_set = int(first[-1])
    still = (np.array([pos[0], pos[1], pos[2], 1], F), nrm, "still")
    if k >= n_st + n_set:
        return zero, nrm, "appeared"
    if k < n_st:
        return still
    t = k - n_st
    o = max(j for j in range(len(first) - 1) if first[j] <= t)
    if prev["visible"][o] == 0:
        return zero, nrm, "appeared"
    if all(_bits(cur["m"][o])[j] == _bits(prev["m"][o])[j] for j in MR.READ):
        return still

    def verts(m):
        out = []
        for j in range(3):
            x, y, z = (F(c) for c in vpos[vidx[3 * t + j]])
            with np.errstate(all="ignore"):
                out.append([F(F(F(F(m[r] * x) + F(m[4 + r] * y)) + F(m[8 + r] * z)) + m[12 + r]) for r in range(3)])
        return out

    def unit(p):
        with np.errstate(all="ignore"):
            e1, e2 = [F(p[1][a] - p[0][a]) for a in range(3)], [F(p[2][a] - p[0][a]) for a in range(3)]
            n = [F(F(e1[1] * e2[2]) - F(e1[2] * e2[1])), F(F(e1[2] * e2[0]) - F(e1[0] * e2[2])),
                 F(F(e1[0] * e2[1]) - F(e1[1] * e2[0]))]
            sq = F(F(F(n[0] * n[0]) + F(n[1] * n[1])) + F(n[2] * n[2]))
            return [F(c / np.sqrt(sq)) for c in n], bool(np.isfinite(sq) and sq > 0)

    pp = verts(np.asarray(prev["m"][o], F))
    with np.errstate(all="ignore"):
        q = [F(fmaf(float(bary[1]), float(F(pp[2][a] - pp[0][a])),
                    float(F(fmaf(float(bary[0]), float(F(pp[1][a] - pp[0][a])), float(pp[0][a])))))) for a in range(3)]
        n_prev, okp = unit(pp)
        n_cur, okc = unit(verts(np.asarray(cur["m"][o], F)))
        flip = F(F(F(n_cur[0] * nrm[0]) + F(n_cur[1] * nrm[1])) + F(n_cur[2] * nrm[2])) < 0
    pn = np.array([-c if flip else c for c in n_prev] + [0], F) if okp and okc else nrm
    if not np.isfinite(q).all():
        return zero, pn, "appeared"
    return np.array(q + [1], F), pn, "moved"


@pytest.mark.parametrize("name", ("catalogue", "seventy"))
def test_hostile_planes_give_the_records_the_rule_names(name):
    meshes, placing = MI.object_set(name)
    vpos, vidx, first = MI.packed(meshes)
    w, h = 33, 23
    hp = MI.hostile_planes(w, h, MI.n_static(), int(first[-1]))
    seen = set()
    for rnd in (0, 3, 7):
        prev, cur = MI.round_poses(placing, rnd)
        _, r = _motion(name, cur, prev, w, h, planes=hp)
        _, r0 = _motion(name, cur, prev, w, h, with_nrm=False, planes=hp)
        assert r0["prev_nrm"] is None and np.array_equal(_bits(r0["motion"]), _bits(r["motion"])) and r0["stats"] == r["stats"]
        count = {"still": 0, "moved": 0, "appeared": 0}
        for y in range(h):
            for x in range(w):
                m, pn, c = _one_pixel(hp["pos"][y, x], hp["nrm"][y, x], int(hp["tri_id"][y, x]), hp["bary"][y, x],
                                      MI.n_static(), first, vpos, vidx, cur, prev)
                assert np.array_equal(_bits(m), _bits(r["motion"][y, x])), (rnd, y, x, c)
                assert np.array_equal(_bits(pn), _bits(r["prev_nrm"][y, x])), (rnd, y, x, c)
                if c:
                    count[c] += 1
                    seen.add((c, bool(np.isfinite(hp["bary"][y, x]).all())))
        assert r["stats"] == (sum(count.values()), count["still"], count["moved"], count["appeared"])
        assert min(count.values()) > 0
    assert ("appeared", False) in seen and ("moved", True) in seen


def test_argument_rule():
    assert MR.check_args(64, 48, 7, 7, True, True) is None and MR.check_args(64, 48, 7, 7, False, False) is None
    for bad in ((0, 48, 7, 7, True, True), (64, 0, 7, 7, True, True), (65537, 1, 7, 7, True, True),
                (65536, 65536, 7, 7, True, True), (64, 48, 6, 7, True, True), (64, 48, 7, 7, True, False),
                (64, 48, 7, 7, False, True)):
        assert MR.check_args(*bad) is not None, bad


# ---- (f) the boundary ------------------------------------------------------------------------------------------------
def test_header_and_binding():
    import ctypes as C
    from vct import Context, _lib, motion, shading, temporal
    src = open(os.path.join(REPO, "include", "vct_motion.h")).read()
    for name in NAMES:
        assert f"vct_status {name}(" in src
    vct_h = open(os.path.join(REPO, "include", "vct.h")).read()
    assert vct_h.count('#include "vct_motion.h"') == 1
    assert vct_h.index('#include "vct_objects.h"') < vct_h.index('#include "vct_motion.h"')
    assert vct_h.index('#include "vct_temporal.h"') < vct_h.index('#include "vct_motion.h"')
    assert "#define VCT_ABI_VERSION 1" in vct_h
    assert _lib.MOTION_EXTENSIONS == NAMES
    assert not set(NAMES) & (set(_lib.EXPORTS) | set(_lib.OBJECTS_EXTENSIONS) | set(_lib.TEMPORAL_EXTENSIONS))
    a = _lib.VctMotionArgs
    assert [f for f, _ in a._fields_] == ["width", "height", "pos4", "nrm4", "tri_id", "bary2", "prev_poses", "n_prev",
                                          "motion4", "prev_nrm4", "stats"]
    assert C.sizeof(a) == 80 and a.prev_poses.offset == 40 and a.n_prev.offset == 48 and a.motion4.offset == 56
    for attr in ("objects_poses_device", "objects_motion_device"):
        assert callable(getattr(Context, attr))
    assert callable(motion.MotionTracker) and callable(shading.set_flat)
    assert "test_normals" in temporal.History.accumulate.__code__.co_varnames


def test_library_exports_the_symbols():
    import ctypes as C
    from vct import _lib
    path = os.path.join(REPO, "voxel-based-global-illumination_amd", "vct", "libvct_hip.so")
    assert os.path.exists(path), "build first (__graft_entry__.build)"
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= exported
    lib = _lib.load()
    for name in NAMES:
        assert _lib.bind_motion_extension(lib, name).restype is C.c_int32
    # a NULL context is VCT_EINVAL from both, before anything is touched
    assert _lib.bind_motion_extension(lib, "vct_objects_poses_device")(None, None, 0) == 1
    assert _lib.bind_motion_extension(lib, "vct_objects_motion_device")(None, None) == 1
