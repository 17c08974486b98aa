"""Reference for vct_inject_lights / vct_composite_lights_device (TEST INFRASTRUCTURE ONLY).

A numpy float32 restatement of include/vct_spec.h "local lights", written from that text:
every step is one float32 numpy operation in the order the spec gives (numpy's float32
+, -, *, / and sqrt are the IEEE operations, correctly rounded; nothing is fused).  All
receivers advance through the shadow walk in lockstep, one cell per iteration.

A light is any object with the fields of `vct_light` (include/vct_lights.h): type,
position, direction, color, range, cos_inner, cos_outer -- the ctypes struct that
vct.point_light() and friends return is one.
"""
from __future__ import annotations

import numpy as np

F = np.float32
DIRECTIONAL, POINT, SPOT = 0, 1, 2
INF = F(np.inf)


def _f3(v):
    return np.array([v[0], v[1], v[2]], dtype=F)


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def prepare(light, n, g0, E):
    """The per-light host constants of the spec."""
    g0 = _f3(g0)
    inv_h = F(n) / F(E)
    hh = F(E) / F(n)
    t = int(light.type)
    out = {"type": t, "color": _f3(light.color)}
    if t == DIRECTIONAL:
        d = _f3(light.direction)
        out["l"] = d / np.sqrt(dot3(d[0], d[1], d[2], d[0], d[1], d[2]))
        return out
    with np.errstate(all="ignore"):                  # overflowing ranges and one-ulp spans are legal
        out["pL"] = (_f3(light.position) - g0) * inv_h
        rv = F(light.range) * inv_h
        out["inv_rr"] = F(1.0) / (rv * rv)
        out["h2"] = hh * hh
        if t == SPOT:
            d = _f3(light.direction)
            out["a"] = -(d / np.sqrt(dot3(d[0], d[1], d[2], d[0], d[1], d[2])))
            out["cos_outer"] = F(light.cos_outer)
            out["inv_span"] = F(1.0) / (F(light.cos_inner) - F(light.cos_outer))
    return out


def evaluate(L, q, N):
    """Per receiver (q, N: [R, 3] float32): l [R, 3], f, ndl, t_lim [R], and the receivers'
    classes before the walk: zero (r2 > 0 fails), back (ndl > 0 fails), culled (f > 0 fails
    where ndl > 0 holds: out of range or outside the cone), walk (the rest)."""
    R = q.shape[0]
    with np.errstate(all="ignore"):
        if L["type"] == DIRECTIONAL:
            l = np.broadcast_to(L["l"], (R, 3)).astype(F)
            f = np.ones(R, F)
            t_lim = np.full(R, INF, F)
            zero = np.zeros(R, bool)
        else:
            d = L["pL"][None, :] - q
            r2 = dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
            zero = ~(r2 > 0)
            r = np.sqrt(r2)
            l = d / r[:, None]
            t_lim = r
            u = r2 * L["inv_rr"]
            w = np.fmax(F(1.0) - u, F(0.0))
            f = (w * w) / (F(1.0) + r2 * L["h2"])
            if L["type"] == SPOT:
                a = L["a"]
                cd = dot3(l[:, 0], l[:, 1], l[:, 2], a[0], a[1], a[2])
                s = np.fmin(np.fmax((cd - L["cos_outer"]) * L["inv_span"], F(0.0)), F(1.0))
                f = f * (s * s)
        ndl = dot3(N[:, 0], N[:, 1], N[:, 2], l[:, 0], l[:, 1], l[:, 2])
        back = ~zero & ~(ndl > 0)
        culled = ~zero & (ndl > 0) & ~(f > 0)
        walk = ~zero & (f > 0) & (ndl > 0)
    return l, f, ndl, t_lim, {"zero": zero, "culled": culled, "back": back, "walk": walk}


def walk_starts(q, n):
    """The shadow-walk receiver rule (vct_spec.h): 0 <= q_a < n in float32 on every axis (a
    NaN fails, -0.0 passes), tested before any conversion.  q: [R, 3] float32 -> [R] bool."""
    q = np.asarray(q, F)
    with np.errstate(all="ignore"):
        return np.all((q >= F(0.0)) & (q < F(n)), axis=1)


def walk(occ, q, l, t_lim, cells=None):
    """A.3 with the t_e >= t_lim end, all receivers in lockstep.  occ: [n, n, n] bool
    (z, y, x).  -> V [R] float32 and the end of every walk: 0 blocked, 1 left the grid
    (or started outside it), 2 reached the light.  A walk starts by the receiver rule
    (`walk_starts`); only a q that passes it is converted to a cell.  cells (an int64 [R]
    array) receives the cells every walk tests."""
    n = occ.shape[0]
    R = q.shape[0]
    V = np.zeros(R, F)
    end = np.zeros(R, np.int8)
    with np.errstate(all="ignore"):
        outside = ~walk_starts(q, n)
        v = np.floor(np.where(outside[:, None], F(0.0), q)).astype(np.int64)
        V[outside] = 1.0
        end[outside] = 1
        s = np.where(l > 0, 1, np.where(l < 0, -1, 0)).astype(np.int64)
        td = np.where(s != 0, F(1.0) / np.abs(l), INF).astype(F)
        # K2 input rule (vct_spec.h): an axis whose td is not finite does not move (s_a = 0,
        # tm_a = +inf), so no t is ever NaN
        s = np.where(td == INF, 0, s)
        vf = v.astype(F)
        tm = np.where(s > 0, ((vf + F(1.0)) - q) * td, np.where(s < 0, (q - vf) * td, INF)).astype(F)
    t_e = np.zeros(R, F)
    act = np.flatnonzero(~outside)
    v, s, td, tm, t_e, t_lim = v[act], s[act], td[act], tm[act], t_e[act], t_lim[act]
    while act.size:
        reached = t_e >= t_lim
        if cells is not None:
            cells[act[~reached]] += 1
        hit = ~reached & occ[v[:, 2], v[:, 1], v[:, 0]]
        V[act[reached]] = 1.0
        end[act[reached]] = 2
        end[act[hit]] = 0
        go = ~(reached | hit)
        # the step: x if tmx <= tmy and tmx <= tmz, else y if tmy <= tmz, else z
        ax = np.where((tm[:, 0] <= tm[:, 1]) & (tm[:, 0] <= tm[:, 2]), 0, np.where(tm[:, 1] <= tm[:, 2], 1, 2))
        rows = np.arange(act.size)
        t_e = tm[rows, ax]
        v[rows, ax] += s[rows, ax]
        with np.errstate(all="ignore"):
            tm[rows, ax] = tm[rows, ax] + td[rows, ax]
        left = go & np.any((v < 0) | (v >= n), axis=1)
        V[act[left]] = 1.0
        end[act[left]] = 1
        keep = go & ~left
        act, v, s, td, tm, t_e, t_lim = act[keep], v[keep], s[keep], td[keep], tm[keep], t_e[keep], t_lim[keep]
    return V, end


def _direct(occ, q, N, A, lights, n, g0, E, stats=None):
    """acc [R, 3] over the lights in list order."""
    acc = np.zeros((q.shape[0], 3), F)
    for k, light in enumerate(lights):
        L = prepare(light, n, g0, E)
        l, f, ndl, t_lim, cls = evaluate(L, q, N)
        w = np.flatnonzero(cls["walk"])
        V, end = walk(occ, q[w], l[w], t_lim[w])
        with np.errstate(all="ignore"):
            contrib = (((A[w] * L["color"][None, :]) * ndl[w, None]) * f[w, None]) * V[:, None]
            acc[w] = acc[w] + contrib
        if stats is not None:
            stats.append({
                "back": int(cls["back"].sum()), "culled": int(cls["culled"].sum()), "zero": int(cls["zero"].sum()),
                "walked": int(w.size), "blocked": int((end == 0).sum()), "left": int((end == 1).sum()),
                "reached": int((end == 2).sum()), "zero_l": int(np.any(l[w] == 0, axis=1).sum()),
            })
    return acc


def receivers(albedo_occ, normal):
    """K2's receivers: (z, y, x) of the occupied voxels, their q, N and A."""
    z, y, x = np.nonzero(albedo_occ[..., 3] != 0)
    N = np.ascontiguousarray(normal[z, y, x, :3], F)
    c = np.stack([x, y, z], axis=1).astype(F)
    q = (c + F(0.5)) + N
    return (z, y, x), q, N, np.ascontiguousarray(albedo_occ[z, y, x, :3], F)


def inject(n, g0, E, albedo_occ, normal, lights, stats=None):
    """Level 0 after vct_inject_lights: [n, n, n, 4] float32 (z, y, x).  stats (a list)
    receives one dict of class counts per light: back-facing, culled by f, zero distance,
    walked -> blocked / left (the grid) / reached (the light), and zero_l, the walked pairs
    with an exact-zero component of l."""
    albedo_occ = np.asarray(albedo_occ, F)
    normal = np.asarray(normal, F)
    occ = albedo_occ[..., 3] != 0
    (z, y, x), q, N, A = receivers(albedo_occ, normal)
    r0 = np.zeros((n, n, n, 4), F)
    r0[z, y, x, :3] = _direct(occ, q, N, A, lights, n, g0, E, stats)
    r0[z, y, x, 3] = 1.0
    return r0


def composite(n, g0, E, albedo_occ, pos4, nrm4, alb4, diffuse4, spec4, lights, stats=None):
    """The linear output of vct_composite_lights_device: [h, w, 4] float32."""
    occ = np.asarray(albedo_occ, F)[..., 3] != 0
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
    direct = _direct(occ, q, N, A, lights, n, g0, E, stats)
    out[fy, fx, :3] = (direct + A * D[fy, fx, :3]) + S[fy, fx, :3]
    out[fy, fx, 3] = 1.0
    return out


def light_set_s(n):
    """The seven lights the GPU tests put into the Cornell box on scenes.grid_for_unit_box(n):
    a room light, a short-range light (range culling), a ceiling spot, a light outside the
    grid shining through the open front, a light inside the short box (every walk but one
    blocked), a light at a voxel centre (exact-zero components of l), and the directional."""
    import vct
    from vct import scenes
    g0, E = scenes.grid_for_unit_box(n)
    hh = F(E) / F(n)
    centre = [float(F(g) + (F(n // 2) + F(0.5)) * hh) for g in g0]
    return [
        vct.point_light((0.0, 0.6, 0.1), (4.0, 4.0, 4.0), 2.5),
        vct.point_light((-0.35, -0.7, 0.45), (1.0, 0.5, 0.2), 0.9),
        vct.spot_light((0.0, 0.95, 0.0), (0.2, -1.0, 0.1), (6.0, 6.0, 5.0), 3.0, cos_inner=0.9397, cos_outer=0.8192),
        vct.point_light((0.3, 0.2, 4.0), (9.0, 9.0, 9.0), 8.0),
        vct.point_light((0.35, -0.7, 0.3), (2.0, 2.0, 2.0), 2.0),
        vct.point_light(centre, (1.0, 1.0, 1.0), 3.0),
        vct.directional_light(scenes.LIGHT_DIR, (0.5, 0.5, 0.5)),
    ]


_cornell = {}


def cornell(n):
    """Cornell at n^3 on the CPU oracle, computed once: grid (oracle.pipeline's dict), the
    light set S, its reference level 0 and the per-light class counts."""
    if n not in _cornell:
        from oracle import oracle as O
        from vct import scenes
        s = scenes.cornell()
        arrays = s.arrays()
        g0, E = scenes.grid_for_unit_box(n)
        grid = O.pipeline(n, g0, E, *arrays, scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
        lights, stats = light_set_s(n), []
        r0 = inject(n, g0, E, grid["albedo_occ"], grid["normal"], lights, stats)
        for a in (r0, grid["albedo_occ"], grid["normal"], grid["r0"]):
            a.setflags(write=False)
        _cornell[n] = {"scene": s, "arrays": arrays, "g0": g0, "E": E, "grid": grid, "lights": lights,
                       "level0": r0, "stats": stats}
    return _cornell[n]


def bits_equal(a, b) -> bool:
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
