"""Reference for vct_voxel_pick_device / vct_voxel_view_device (TEST INFRASTRUCTURE ONLY).

A numpy float32 restatement of include/vct_spec.h "voxel view", written from that text: every
step is one float32 numpy operation in the order the spec gives; the spec's fused operations go
through shadow_ref.fmaf.  The rays of a call advance in lockstep, one cell per iteration.

What is reused, not restated: the origin and the slab are fog_ref's (`origin`, `slab`, the slab
called with one origin per ray), the pixel ray is gbuffer_ref's, dot3 is lights_ref's, the present
step's tone curve is sky_view_ref's (fog_ref.apply's), the pyramid is query_ref's.  The cell walk
itself cannot be lights_ref.walk: that one returns a visibility and how the walk ended, and a hit
record needs the cell, the entry face, the entry time and the count, which it does not keep.
`walk` below is written from the same rule ("K2 input rule", Walk) and tests/test_voxview.py pins
it to lights_ref.walk on the hostile catalogue: a hit exists exactly where that walk returns 0.

The second half is a float64 caster over the union of the solid cells' boxes with a per-ray
robustness margin, for the comparison that does not depend on float32 rounding.
"""
from __future__ import annotations

import numpy as np

import fog_ref
import gbuffer_ref
import lights_ref
import sky_view_ref
from lights_ref import F
from shadow_ref import fmaf

INF = F(np.inf)
NAN = F(np.nan)
OCCUPANCY, ALPHA = 0, 1                                  # VCT_VOXPICK_*
RADIANCE, MODE_ALPHA, ALBEDO, NORMAL = 0, 1, 2, 3        # VCT_VOXVIEW_*
MODE_NAMES = ("radiance", "alpha", "albedo", "normal")
FACE_INSIDE, FACE_MISS, CELL_MISS = 6, 7, 0xFFFFFFFF
SHADE = (F(0.8), F(1.0), F(0.6), F(1.0))                 # VCT_VOXVIEW_SHADE_X / _Y / _Z, and face 6
STEPS_PER_CELL = 3                                       # VCT_VOXVIEW_STEPS_PER_CELL
INF_BITS = 0x7F800000


# ---- what is solid -----------------------------------------------------------------------------
def solid_occupancy(albedo_occ):
    """K1's occupancy bits: [n, n, n] bool (z, y, x)."""
    return np.asarray(albedo_occ, F)[..., 3] != 0


def solid_alpha(pyr, level):
    """alpha > 0 in any face of the level's texel (a NaN is not solid): [n_l, n_l, n_l] bool.
    pyr: query_ref.pyramid's dict."""
    with np.errstate(invalid="ignore"):
        return np.any(np.stack([v[..., 3] for v in pyr[level]]) > 0, axis=0)


# ---- the walk ----------------------------------------------------------------------------------
def directions(v):
    """The K2 direction rule: -> len [R], d [R, 3]."""
    v = np.asarray(v, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        ln = np.sqrt(lights_ref.dot3(v[:, 0], v[:, 1], v[:, 2], v[:, 0], v[:, 1], v[:, 2]))
        return ln, (v / ln[:, None]).astype(F)


def walk(solid, level, o, v, t_lim):
    """R rays through `solid` ([n_l, n_l, n_l] bool, z y x) of level `level`: o [R, 3] the origins
    in level-0 voxel units, v [R, 3] the directions as given, t_lim [R].
    -> dict(hit4 [R, 4] uint32 records, cell, face, steps (int64), t (float32), d [R, 3])."""
    nl = solid.shape[0]
    nf = F(nl)
    o = np.asarray(o, F).reshape(-1, 3)
    t_lim = np.broadcast_to(np.asarray(t_lim, F), (o.shape[0],))
    R = o.shape[0]
    down, up = F(2.0 ** -level), F(2.0 ** level)
    cell = np.full(R, CELL_MISS, np.int64)
    face = np.full(R, FACE_MISS, np.int64)
    steps = np.zeros(R, np.int64)
    t = np.full(R, INF, F)
    with np.errstate(all="ignore"):
        ln, d = directions(v)
        ll = (np.where(np.isnan(t_lim), INF, t_lim) * down).astype(F)
        ol = (o * down).astype(F)
        ray = (ln > 0) & np.isfinite(ln) & np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
        t0, _, seg, _ = fog_ref.slab(nl, ol.T, d, ll)
        t0 = (t0 + F(0.0)).astype(F)                                # a zero t0 is +0
        # the axis of t0: the first clipping axis whose tn equals it (none for t0 == 0)
        a0 = np.full(R, -1, np.int64)
        for c in (2, 1, 0):
            inv = F(1.0) / d[:, c]
            clip = (d[:, c] != 0) & np.isfinite(inv)
            tn = np.fmin((F(0.0) - ol[:, c]) * inv, (nf - ol[:, c]) * inv)
            a0 = np.where(clip & (t0 > 0) & (tn == t0), c, a0)
        s = np.where(d > 0, 1, np.where(d < 0, -1, 0)).astype(np.int64)
        td = np.where(s != 0, F(1.0) / np.abs(d), INF).astype(F)
        s = np.where(td == INF, 0, s)
        p = (ol + d * t0[:, None]).astype(F)
        vf = np.fmin(np.fmax(np.floor(p), F(0.0)), nf - F(1.0)).astype(F)
        vi = np.where(np.isnan(vf), 0, vf).astype(np.int64)
        vf = vi.astype(F)
        tm = np.where(s > 0, ((vf + F(1.0)) - p) * td, np.where(s < 0, (p - vf) * td, INF)).astype(F)
    rows = np.arange(R)
    fc = np.where(a0 < 0, FACE_INSIDE, 2 * a0 + np.where(s[rows, np.maximum(a0, 0)] > 0, 0, 1))
    act = np.flatnonzero(ray & seg)
    vi, s, td, tm, fc, t0, ll = vi[act], s[act], td[act], tm[act], fc[act], t0[act], ll[act]
    te = t0.copy()
    for _ in range(STEPS_PER_CELL * nl):
        if not act.size:
            break
        steps[act] += 1
        hit = solid[vi[:, 2], vi[:, 1], vi[:, 0]]
        k = act[hit]
        cell[k] = vi[hit, 0] + nl * (vi[hit, 1] + nl * vi[hit, 2])
        face[k] = fc[hit]
        with np.errstate(all="ignore"):
            t[k] = te[hit] * up
            ax = np.where((tm[:, 0] <= tm[:, 1]) & (tm[:, 0] <= tm[:, 2]), 0, np.where(tm[:, 1] <= tm[:, 2], 1, 2))
            r = np.arange(act.size)
            tn = (t0 + tm[r, ax]).astype(F)
            limit = tn >= ll
            vi[r, ax] += s[r, ax]
            left = np.any((vi < 0) | (vi >= nl), axis=1)
            tm[r, ax] = tm[r, ax] + td[r, ax]
        fc = 2 * ax + np.where(s[r, ax] > 0, 0, 1)
        te = tn
        keep = ~(hit | limit | left)
        act, vi, s, td, tm, fc, t0, ll, te = (a[keep] for a in (act, vi, s, td, tm, fc, t0, ll, te))
    hit4 = np.stack([cell.astype(np.uint32), face.astype(np.uint32), steps.astype(np.uint32), t.view(np.uint32)], axis=1)
    return {"hit4": hit4, "cell": cell, "face": face, "steps": steps, "t": t, "d": d, "hit": cell != CELL_MISS}


def pick(n, g0, E, solid, level, org, dirv, t_lim=INF):
    """vct_voxel_pick_device: org, dirv [R, 3] (world), t_lim [R] or a scalar -> walk's dict."""
    org = np.asarray(org, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        o = fog_ref.origin(n, g0, E, org)
    return walk(solid, level, o, dirv, t_lim)


# ---- the view ----------------------------------------------------------------------------------
def quant8(c):
    """q(v) without the tone curve on [..., 3] float32 -> packed uint32, alpha 255."""
    with np.errstate(all="ignore"):
        v = np.asarray(c, F) * F(255.0)
        q = np.clip(np.where(np.isnan(v), 0, np.floor(v.astype(np.float64) + 0.5)), 0, 255).astype(np.uint32)
    return (q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | np.uint32(255 << 24)).astype(np.uint32)


def colours(res, level, mode, pyr=None, aniso=True, albedo_occ=None, normal=None):
    """The colour of every hit cell of `res` (walk's dict) by mode, before the shade: [R, 3]."""
    R = res["cell"].shape[0]
    out = np.zeros((R, 3), F)
    k = np.flatnonzero(res["hit"])
    if mode in (ALBEDO, NORMAL):
        n = albedo_occ.shape[0]
        c = res["cell"][k]
        x, y, z = c % n, (c // n) % n, c // (n * n)
        if mode == ALBEDO:
            out[k] = np.asarray(albedo_occ, F)[z, y, x, :3]
        else:
            out[k] = fmaf(F(0.5), np.asarray(normal, F)[z, y, x, :3], F(0.5))
        return out
    nl = pyr[level][0].shape[0]
    c = res["cell"][k]
    x, y, z = c % nl, (c // nl) % nl, c // (nl * nl)
    if level != 0 and aniso:
        d = res["d"][k]
        vols = np.stack(pyr[level])
        fidx = np.where(d >= 0, 0, 1) + np.array([0, 2, 4])[None, :]
        wd = d * d
        tx, ty, tz = (vols[fidx[:, a], z, y, x] for a in range(3))
        with np.errstate(all="ignore"):
            T = fmaf(wd[:, 2:3], tz, fmaf(wd[:, 1:2], ty, wd[:, 0:1] * tx))
    else:
        T = pyr[level][0][z, y, x]
    out[k] = T[:, 3:4] if mode == MODE_ALPHA else T[:, :3]
    return out


def view(n, g0, E, cam, w, h, level, mode, shade, pyr=None, aniso=True, albedo_occ=None, normal=None):
    """vct_voxel_view_device: -> dict(linear4 [h, w, 4] float32, rgba8 [h, w] uint32,
    hit4 [h, w, 4] uint32, cells (int), res: walk's dict over the h * w rays in row order)."""
    solid = solid_alpha(pyr, level) if mode in (RADIANCE, MODE_ALPHA) else solid_occupancy(albedo_occ)
    dirv = gbuffer_ref.pixel_rays(cam, w, h).reshape(-1, 3)
    o = fog_ref.origin(n, g0, E, np.asarray(cam.position, F))
    res = walk(solid, level, np.broadcast_to(o, dirv.shape), dirv, INF)
    C = colours(res, level, mode, pyr, aniso, albedo_occ, normal)
    if shade:
        with np.errstate(all="ignore"):
            C = (C * np.array(SHADE, F)[np.minimum(res["face"] >> 1, 3)][:, None]).astype(F)
    hit = res["hit"]
    lin = np.zeros((h * w, 4), F)
    lin[hit, :3] = C[hit]
    lin[hit, 3] = 1.0
    q = np.zeros(h * w, np.uint32)
    q[hit] = (sky_view_ref.tone8(C) if mode == RADIANCE else quant8(C))[hit]
    return {"linear4": lin.reshape(h, w, 4), "rgba8": q.reshape(h, w), "hit4": res["hit4"].reshape(h, w, 4),
            "cells": int(res["steps"].sum()), "res": res}


def view_rays(cam, w, h):
    """The pick list that equals the view of `cam`: org [h * w, 3], dir [h * w, 3] (t_lim = +inf)."""
    dirv = gbuffer_ref.pixel_rays(cam, w, h).reshape(-1, 3)
    return np.broadcast_to(np.asarray(cam.position, F), dirv.shape).copy(), dirv


# ---- the float64 caster ------------------------------------------------------------------------
EPS64 = 1e-3          # voxel units of the level: the margin every robust decision keeps


def cast64(solid, level, o, v, eps=EPS64):
    """The nearest intersection of R rays with the union of the solid cells' boxes, in float64:
    o [R, 3] (level-0 voxel units), v [R, 3].  -> cell, face (CELL_MISS / FACE_MISS for a miss),
    t (level units) and robust [R]: the winner's entry time is more than eps from the entry time
    of every other cell the ray may touch and from its own exit, its two latest slab entries
    are more than eps apart (the face is not in doubt), an origin is more than eps inside or
    outside its cell, and no cell is within eps of being hit at all before the winner."""
    nl = solid.shape[0]
    o = np.asarray(o, np.float64).reshape(-1, 3) * 2.0 ** -level
    v = np.asarray(v, np.float64).reshape(-1, 3)
    d = v / np.linalg.norm(v, axis=1)[:, None]
    z, y, x = np.nonzero(solid)
    lo = np.stack([x, y, z], axis=1).astype(np.float64)             # [S, 3]
    R, S = o.shape[0], lo.shape[0]
    cell = np.full(R, CELL_MISS, np.int64)
    face = np.full(R, FACE_MISS, np.int64)
    t = np.full(R, np.inf)
    robust = np.ones(R, bool)
    if S == 0:
        return cell, face, t, robust
    with np.errstate(all="ignore"):
        inv = 1.0 / d                                               # +-inf for a zero component
        ta = (lo[None, :, :] - o[:, None, :]) * inv[:, None, :]     # [R, S, 3]
        tb = (lo[None, :, :] + 1.0 - o[:, None, :]) * inv[:, None, :]
        par = (d == 0)[:, None, :]
        inside_par = (o[:, None, :] >= lo[None, :, :]) & (o[:, None, :] <= lo[None, :, :] + 1.0)
        tn = np.where(par, np.where(inside_par, -np.inf, np.inf), np.minimum(ta, tb))
        tf = np.where(par, np.where(inside_par, np.inf, -np.inf), np.maximum(ta, tb))
    enter, leave = tn.max(axis=2), tf.min(axis=2)                   # [R, S]
    start = np.maximum(enter, 0.0)
    margin = leave - start                                          # > 0: the ray passes through the box
    touched = margin > 0
    maybe = margin > -eps
    key = np.where(touched, start, np.inf)
    win = key.argmin(axis=1)
    r = np.arange(R)
    has = touched[r, win]
    t_win = np.where(has, key[r, win], np.inf)
    cell[has] = (x[win] + nl * (y[win] + nl * z[win]))[has]
    tnw = tn[r, win]
    axis = tnw.argmax(axis=1)
    inside = enter[r, win] < 0
    face[has] = np.where(inside, FACE_INSIDE, 2 * axis + np.where(d[r, axis] > 0, 0, 1))[has]
    t[has] = t_win[has]
    # robustness
    others = maybe.copy()
    others[r, win] &= ~has
    first_other = np.where(others, start, np.inf).min(axis=1)
    robust &= np.where(has, first_other > t_win + eps, ~others.any(axis=1))   # a miss: no cell may be touched at all
    srt = np.sort(tnw, axis=1)
    robust &= ~has | (margin[r, win] > eps)
    robust &= ~has | inside | (srt[:, 2] - srt[:, 1] > eps)
    robust &= ~has | (np.abs(enter[r, win]) > eps)
    return cell, face, t, robust


# ---- the inputs the CPU and GPU tests share ----------------------------------------------------
def cameras():
    """The three cameras of the Cornell frames: an eye outside the grid, one inside the box, an
    oblique one outside."""
    from vct.camera import Camera
    return {"outside": Camera((0.0, 0.0, 4.0)),
            "inside": Camera(fog_ref.EYE_IN, yaw=-70.0, pitch=-12.0),
            "oblique": Camera((1.7, 1.3, 2.4), yaw=-124.0, pitch=-24.0)}


def hostile_rays(n, g0, E):
    """Hand-made rays on an n^3 grid, (name, org (world), dir, t_lim): every class of the spec's
    rule.  World points are formed from voxel coordinates as g0 + q * (E / n) in float32."""
    g0 = np.asarray(g0, F)
    hh = F(E) / F(n)

    def W(q):
        return (g0 + np.asarray(q, F) * hh).astype(F)

    c = F(n) / F(2)
    big = F(3.0e38)
    rows = [
        ("axis +x", W((-2.0, c + 0.5, c + 0.5)), (1.0, 0.0, 0.0), INF),
        ("axis -y -0", W((c + 0.5, n + 3.0, c + 0.5)), (-0.0, -2.5, 0.0), INF),
        ("axis +z inside", W((c + 0.5, c + 0.5, c + 0.5)), (0.0, 0.0, 1e-30), INF),
        ("diagonal through corners", W((-1.0, -1.0, -1.0)), (1.0, 1.0, 1.0), INF),
        ("diagonal back", W((n + 1.0, n + 1.0, n + 1.0)), (-3.0, -3.0, -3.0), INF),
        ("tiny x", W((c + 0.25, n + 2.0, c + 0.25)), (2.0 ** -130, -1.0, 0.0), INF),
        ("tiny x outside its slab", W((-0.5, n + 2.0, c + 0.25)), (2.0 ** -130, -1.0, 0.0), INF),
        ("on the face", W((0.0, c + 0.5, c + 0.5)), (1.0, 0.1, 0.2), INF),
        ("on the corner", W((0.0, 0.0, 0.0)), (1.0, 0.9, 0.8), INF),
        ("on the far corner, leaving", W((float(n), float(n), float(n))), (1.0, 1.0, 1.0), INF),
        ("outside, pointing away", W((-3.0, c, c)), (-1.0, 0.2, 0.1), INF),
        ("limit 0", W((c + 0.5, c + 0.5, c + 0.5)), (0.3, -1.0, 0.2), F(0.0)),
        ("limit negative", W((c + 0.5, c + 0.5, c + 0.5)), (0.3, -1.0, 0.2), F(-1.0)),
        ("limit nan", W((c + 0.5, c + 0.5, c + 0.5)), (0.3, -1.0, 0.2), NAN),
        ("limit short", W((c + 0.5, c + 0.5, c + 0.5)), (0.3, -1.0, 0.2), F(1.25)),
        ("limit before the grid", W((-4.0, c + 0.5, c + 0.5)), (1.0, 0.0, 0.0), F(3.5)),
        ("zero direction", W((c, c, c)), (0.0, -0.0, 0.0), INF),
        ("nan direction", W((c, c, c)), (0.3, np.nan, 0.1), INF),
        ("inf direction", W((c, c, c)), (np.inf, 0.0, 0.0), INF),
        ("overflowing direction", W((c, c, c)), (big, big, 0.0), INF),
        ("underflowing direction", W((c, c, c)), (1e-30, -1e-30, 1e-30), INF),
        ("nan origin", (np.nan, 0.0, 0.0), (0.0, 0.0, -1.0), INF),
        ("inf origin", (0.0, -np.inf, 0.0), (0.0, 1.0, 0.0), INF),
        ("overflowing origin", (big, 0.0, 0.0), (-1.0, 0.0, 0.0), INF),
        ("far origin", (1.0e18, 0.1, 0.2), (-1.0, 0.0, 0.0), INF),
    ]
    org = np.array([np.asarray(r[1], F) for r in rows], F)
    dirv = np.array([r[2] for r in rows], F)
    lim = np.array([r[3] for r in rows], F)
    return [r[0] for r in rows], org, dirv, lim
