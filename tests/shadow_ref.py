"""Reference for vct_shadow_cones_device / vct_composite_shadowed_device (TEST INFRASTRUCTURE ONLY).

A numpy float32 restatement of include/vct_spec.h "shadow cones", written from that text.
The receivers of one light advance through the march in lockstep, one step per iteration:
(t, D, l0, fr) depend only on the aperture and the step index, so they are scalars (exact
binary32 through spec_ref's scalar helpers), and everything per receiver is one float32
numpy operation in the order the spec gives.  The spec's fused operations go through
:func:`fmaf`, an exact vectorised binary32 fma.

The per-light terms, the skip rule and the hard walk are tests/lights_ref.py's (the walk under
the K2 input rule of vct_spec.h: an axis whose td is not finite does not move; its start under
the shadow-walk receiver rule: V = 1 without a walk unless 0 <= q < n in float32).
"""
from __future__ import annotations

import numpy as np

import lights_ref
import spec_ref
from lights_ref import F, _f3

ALPHA_STOP = F(spec_ref.ALPHA_STOP)
END_ALPHA, END_LEFT, END_REACHED = 0, 1, 2        # how a marched pair ended
END_NAMES = ("alpha stop", "left grid", "light reached")


def fmaf(a, b, c):
    """Correctly rounded binary32 a * b + c, element-wise.  The product of two binary32
    values is exact in binary64; TwoSum gives the sum's rounding error; the binary64 sum is
    then forced to round-to-odd (inexact: its last bit is set), after which the cast to
    binary32 rounds once (53 >= 24 + 2 bits)."""
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        s, err = np.broadcast_arrays(s, err)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(fix, odd, s).astype(F)


def alpha_pyramid(n, level0, aniso=True):
    """{level: [nl, nl, nl] alpha volumes (z, y, x), one per face} of the pyramid K3 builds
    from `level0` (the CPU oracle's build)."""
    from oracle import oracle as O
    O.build()
    level0 = np.ascontiguousarray(level0, F)
    out = {0: [np.ascontiguousarray(level0[..., 3])]}
    levels = O.pyramid_levels(n, O.build_mips(n, level0, aniso), aniso)
    for l, vols in levels.items():
        out[l] = [np.ascontiguousarray(v[..., 3]) for v in vols]
    return out


def step_rows(tau, n):
    """The (t, D, l0, fr) of every step an unlimited cone of aperture tau can take."""
    f32 = spec_ref.f32
    L = int(round(np.log2(n)))
    tau2 = f32(2.0 * tau)
    tmax = f32(f32(n) * spec_ref.SQRT3)
    t, rows = 1.0, []
    while t <= tmax:
        D = max(1.0, f32(tau2 * t))
        m = min(spec_ref.log2(D), float(L))
        l0 = int(m)
        rows.append((F(t), l0, F(f32(m - l0))))
        t = f32(t + f32(spec_ref.STEP_SCALE * D))
    return rows


def _sample(alpha, l, aniso, p, face, d2, n):
    """The alpha of D_l(p, d) for every receiver (A.5): p [R, 3], face [R, 3] the face index
    per axis, d2 [R, 3] the face weights."""
    nl = n >> l
    scale = F(2.0 ** -l)
    c = p * scale - F(0.5)
    fl = np.floor(c)
    i0 = fl.astype(np.int64)
    w1 = c - fl
    w = (F(1.0) - w1, w1)
    acc = np.zeros(p.shape[0], F)
    faces = l != 0 and aniso
    vols = np.stack(alpha[l]) if faces else alpha[l][0]
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                x, y, z = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
                inside = (x >= 0) & (x < nl) & (y >= 0) & (y < nl) & (z >= 0) & (z < nl)
                xc, yc, zc = (np.clip(v, 0, nl - 1) for v in (x, y, z))
                wc = (w[dx][:, 0] * w[dy][:, 1]) * w[dz][:, 2]
                if faces:
                    fx, fy, fz = (vols[face[:, k], zc, yc, xc] for k in range(3))
                    v = fmaf(d2[:, 2], fz, fmaf(d2[:, 1], fy, d2[:, 0] * fx))
                else:
                    v = vols[zc, yc, xc]
                v = np.where(inside, v, F(0.0)).astype(F)
                acc = fmaf(wc, v, acc)
    return acc


def march(alpha, n, aniso, o, d, t_lim, tau):
    """Steps 1-5 of the spec for R cones: o, d [R, 3], t_lim [R], one clamped aperture tau.
    -> a [R] float32, steps [R], end [R] (END_*; the t > t_max end counts as END_LEFT)."""
    L = int(round(np.log2(n)))
    R = o.shape[0]
    o, d, t_lim = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F), np.ascontiguousarray(t_lim, F)
    a = np.zeros(R, F)
    steps = np.zeros(R, np.int64)
    end = np.full(R, END_LEFT, np.int8)
    face = np.where(d >= 0, 0, 1) + np.array([0, 2, 4])[None, :]
    d2 = d * d
    act = np.arange(R)
    nf = F(n)
    for t, l0, fr in step_rows(tau, n):
        if not act.size:
            break
        stop = ~(a[act] < ALPHA_STOP)
        end[act[stop]] = END_ALPHA
        act = act[~stop]
        reached = t >= t_lim[act]
        end[act[reached]] = END_REACHED
        act = act[~reached]
        p = o[act] + d[act] * t
        inside = np.all((p >= 0) & (p <= nf), axis=1)
        end[act[~inside]] = END_LEFT
        act, p = act[inside], p[inside]
        if not act.size:
            break
        s = _sample(alpha, l0, aniso, p, face[act], d2[act], n)
        if fr > 0 and l0 < L:
            s1 = _sample(alpha, l0 + 1, aniso, p, face[act], d2[act], n)
            s = fmaf(fr, s1, (F(1.0) - fr) * s)
        a[act] = fmaf(F(1.0) - a[act], s, a[act])
        steps[act] += 1
    # cones still marching when the table ends: the ends the spec tests before t <= t_max
    stop = ~(a[act] < ALPHA_STOP)
    end[act[stop]] = END_ALPHA
    return a, steps, end


def visibility(a):
    return np.fmax(F(1.0) - np.asarray(a, F) / ALPHA_STOP, F(0.0)).astype(F)


def clamp_tau(tan_half):
    return float(np.fmin(np.fmax(F(tan_half), F(spec_ref.TAU_MIN)), F(spec_ref.TAU_MAX)))


def shadow(n, g0, E, albedo_occ, alpha, aniso, pos4, nrm4, lights, tan_half):
    """vct_shadow_cones_device: -> dict(vis [n_lights, h, w] float32, steps (int), pairs: per
    light dict(px: flat pixel indices of the pairs not skipped, V, end (None for a hard
    light), soft))."""
    occ = np.asarray(albedo_occ, F)[..., 3] != 0
    pos4, nrm4 = np.asarray(pos4, F), np.asarray(nrm4, F)
    h, w = pos4.shape[:2]
    vis = np.zeros((len(lights), h, w), F)
    fy, fx = np.nonzero(pos4[..., 3] != 0)
    P, N = pos4[fy, fx, :3], nrm4[fy, fx, :3]
    inv_h = F(n) / F(E)
    with np.errstate(all="ignore"):                  # a pixel's position and normal may hold anything
        q = (P - _f3(g0)[None, :]) * inv_h + N
    total, pairs = 0, []
    for j, light in enumerate(lights):
        Lc = lights_ref.prepare(light, n, g0, E)
        l, f, ndl, t_lim, cls = lights_ref.evaluate(Lc, q, N)
        k = np.flatnonzero(cls["walk"])
        if F(tan_half[j]) == 0:
            V, _ = lights_ref.walk(occ, q[k], l[k], t_lim[k])
            end = None
        else:
            a, steps, end = march(alpha, n, aniso, q[k], l[k], t_lim[k], clamp_tau(tan_half[j]))
            V = visibility(a)
            total += int(steps.sum())
        vis[j, fy[k], fx[k]] = V
        pairs.append({"px": fy[k] * w + fx[k], "V": V, "end": end, "soft": end is not None})
    return {"vis": vis, "steps": total, "pairs": pairs}


def composite(n, g0, E, pos4, nrm4, alb4, diffuse4, spec4, lights, vis):
    """The linear output of vct_composite_shadowed_device: [h, w, 4] float32."""
    pos4, nrm4, alb4 = (np.asarray(a, F) for a in (pos4, nrm4, alb4))
    D, S = np.asarray(diffuse4, F), np.asarray(spec4, F)
    h, w = pos4.shape[:2]
    out = np.empty((h, w, 4), F)
    out[...] = np.array([0.2, 0.3, 0.3, 0.0], F)                   # VCT_CLEAR_*, alpha 0
    fy, fx = np.nonzero(pos4[..., 3] != 0)
    P, N, A = pos4[fy, fx, :3], nrm4[fy, fx, :3], alb4[fy, fx, :3]
    inv_h = F(n) / F(E)
    with np.errstate(all="ignore"):                  # a pixel's position and normal may hold anything
        q = (P - _f3(g0)[None, :]) * inv_h + N
    acc = np.zeros((q.shape[0], 3), F)
    for j, light in enumerate(lights):
        Lc = lights_ref.prepare(light, n, g0, E)
        l, f, ndl, t_lim, cls = lights_ref.evaluate(Lc, q, N)
        k = np.flatnonzero(cls["walk"])
        V = np.asarray(vis, F)[j, fy[k], fx[k]]
        with np.errstate(all="ignore"):
            acc[k] = acc[k] + (((A[k] * Lc["color"][None, :]) * ndl[k, None]) * f[k, None]) * V[:, None]
    out[fy, fx, :3] = (acc + A * D[fy, fx, :3]) + S[fy, fx, :3]
    out[fy, fx, 3] = 1.0
    return out


# ---- the inputs the CPU and GPU tests share ---------------------------------------------
TAN_HALF = [0.05, 0.2, 0.1, 0.05, 0.3, 0.02, 0.1, 0.0]
FRAMES = {4: (1, 1), 8: (13, 7), 16: (32, 24), 32: (32, 24), 64: (48, 36)}


def lights_for(n):
    """lights_ref.light_set_s(n) followed by its directional light once more (soft, then hard)."""
    s = lights_ref.cornell(n)["lights"]
    return list(s) + [s[-1]]


_alpha = {}


def cornell_alpha(n, aniso=True):
    """The alpha pyramid of lights_ref.cornell(n)'s level 0, computed once."""
    if (n, aniso) not in _alpha:
        _alpha[(n, aniso)] = alpha_pyramid(n, lights_ref.cornell(n)["level0"], aniso)
    return _alpha[(n, aniso)]


def reference(n, pos4, nrm4, aniso=True, lights=None, tan_half=None):
    c = lights_ref.cornell(n)
    return shadow(n, c["g0"], c["E"], c["grid"]["albedo_occ"], cornell_alpha(n, aniso), aniso, pos4, nrm4,
                  lights_for(n) if lights is None else lights, TAN_HALF if tan_half is None else tan_half)


def coverage(ref):
    """Shares over the marched (soft, not skipped) pairs: the three end classes, the
    penumbra 0.05 < V < 0.95, and V == 1 exactly."""
    end = np.concatenate([p["end"] for p in ref["pairs"] if p["soft"]])
    V = np.concatenate([p["V"] for p in ref["pairs"] if p["soft"]])
    m = max(end.size, 1)
    return {"pairs": int(end.size), "alpha stop": float((end == END_ALPHA).sum()) / m,
            "light reached": float((end == END_REACHED).sum()) / m, "left grid": float((end == END_LEFT).sum()) / m,
            "penumbra": float(((V > 0.05) & (V < 0.95)).sum()) / m, "lit": float((V == 1.0).sum()) / m}
