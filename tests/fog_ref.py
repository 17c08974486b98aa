"""Reference for include/vct_fog.h (TEST INFRASTRUCTURE ONLY).

A numpy float32 restatement of include/vct_spec.h "volumetric fog", written from that text:
one float32 numpy operation per spec operation, the fused operations through shadow_ref.fmaf.
It composes what the other references already pin: a light's constants and attenuation are
lights_ref's (prepare / evaluate with the cell centre as the receiver; the cosine it also
returns is not used), a light's visibility is shadow_ref.march from the cell centre, and the
ambient term is the CPU oracle's K4 (oracle.trace, diffuse cones only) on the synthetic
records.  Rays, slab, trilinear and compositing are restated directly; all rays advance
through the march in lockstep, one sample per iteration.

A fog is a dict(density, albedo, ambient, level, step).
"""
from __future__ import annotations

import ctypes

import numpy as np

import lights_ref
import shadow_ref
from shadow_ref import fmaf

F = np.float32
INF = F(np.inf)
PHASE = F(0.0795774715)          # VCT_FOG_PHASE
T_STOP = F(0.00390625)           # VCT_FOG_T_STOP
MAX_STEPS = 4096                 # VCT_FOG_MAX_STEPS
DENSITY_LIMIT = F(2.0 ** 20)     # VCT_FOG_DENSITY_LIMIT

END_SAMPLES, END_TSTOP, END_EMPTY, END_NULL = 0, 1, 2, 3      # how a ray ended
END_NAMES = ("out of samples", "T stop", "clipped empty", "null record")
SKIP_NONE, SKIP_ZERO, SKIP_RANGE, SKIP_CONE = 0, 1, 2, 3      # why a (cell, light) pair marched no cone
SKIP_NAMES = ("marched", "zero distance", "out of range", "outside the cone")


def fog(density, albedo=(1.0, 1.0, 1.0), ambient=0.0, level=1, step=1.0):
    return {"density": density, "albedo": tuple(albedo), "ambient": ambient, "level": level, "step": step}


def to_ctypes(f):
    import vct
    return vct.fog(f["density"], f["albedo"], f["ambient"], f["level"], f["step"])


def sigma_v(f, n, E):
    """sigma_v = (density * E) / (float)n."""
    return (F(f["density"]) * F(E)) / F(n)


def cell_centres(n, level):
    """-> x_c [m^3, 3] float32 in the volume's linear order (z, y, x; x fastest), m."""
    m = n >> level
    cs = F(2.0 ** level)
    c = (np.arange(m, dtype=F) + F(0.5)) * cs
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(F), m


# ---- the scatter volume -----------------------------------------------------------------------
def ambient_records(n, g0, E, level):
    """The synthetic G-buffer of the ambient term: (pos4, nrm4, alb4) of shape [2 m^2, m, 4];
    the first m^2 rows are the +y records in the cells' linear order, the rest the -y records."""
    xc, m = cell_centres(n, level)
    hh = F(E) / F(n)
    P = np.array(g0, F)[None, :] + xc * hh
    pos = np.ones((2 * m ** 3, 4), F)
    pos[:, :3] = np.concatenate([P, P])
    nrm = np.zeros((2 * m ** 3, 4), F)
    nrm[: m ** 3, 1], nrm[m ** 3:, 1] = 1.0, -1.0
    alb = np.zeros((2 * m ** 3, 4), F)
    shape = (2 * m * m, m, 4)
    return pos.reshape(shape), nrm.reshape(shape), alb.reshape(shape)


def ambient(n, g0, E, level0, level, aniso=True, n_diffuse=9):
    """A [m^3, 3] = 0.5 (I+ + I-) from the CPU oracle's K4 on the synthetic records."""
    from oracle import oracle as O
    O.build()
    xc, m = cell_centres(n, level)
    if n_diffuse == 0:
        return np.zeros((m ** 3, 3), F)
    level0 = np.ascontiguousarray(level0, F)
    pyr = O.build_mips(n, level0, aniso)
    pos, nrm, alb = ambient_records(n, g0, E, level)
    out = O.trace(n, g0, E, level0, pyr, pos, nrm, alb, (0.0, 0.0, 0.0), aniso=aniso, n_diffuse=n_diffuse,
                  specular=False)
    I = np.ascontiguousarray(out["diffuse"], F).reshape(2, m ** 3, 4)[..., :3]
    return (F(0.5) * (I[0] + I[1])).astype(F)


def build(n, g0, E, alpha, aniso, f, lights, tan_half, A=None):
    """vct_build_fog: -> dict(S [m, m, m, 4], acc [m^3, 3], V / att / skip [n_lights, m^3], steps).
    alpha: shadow_ref.alpha_pyramid of the level 0; A: ambient()'s array when f['ambient'] > 0."""
    xc, m = cell_centres(n, f["level"])
    R = xc.shape[0]
    acc = np.zeros((R, 3), F)
    Vs = np.full((len(lights), R), np.nan, F)
    atts = np.zeros((len(lights), R), F)
    skip = np.zeros((len(lights), R), np.int8)
    steps = 0
    dummy = np.zeros((R, 3), F)
    for j, light in enumerate(lights):
        L = lights_ref.prepare(light, n, g0, E)
        l, att, _, t_lim, cls = lights_ref.evaluate(L, xc, dummy)
        with np.errstate(all="ignore"):
            go = ~cls["zero"] & (att > 0)
            if L["type"] != lights_ref.DIRECTIONAL:
                d = L["pL"][None, :] - xc
                r2 = lights_ref.dot3(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
                w = np.fmax(F(1.0) - r2 * L["inv_rr"], F(0.0))
                skip[j] = np.where(cls["zero"], SKIP_ZERO, np.where(go, SKIP_NONE, np.where(w > 0, SKIP_CONE, SKIP_RANGE)))
        k = np.flatnonzero(go)
        a, st, _ = shadow_ref.march(alpha, n, aniso, xc[k], l[k], t_lim[k], shadow_ref.clamp_tau(tan_half[j]))
        V = shadow_ref.visibility(a)
        steps += int(st.sum())
        Vs[j, k], atts[j, k] = V, att[k]
        wgt = att[k] * V
        acc[k] = fmaf(L["color"][None, :], wgt[:, None], acc[k])
    S = PHASE * acc
    amb = F(f["ambient"])
    if amb > 0:
        S = fmaf(amb, np.zeros((R, 3), F) if A is None else np.asarray(A, F), S)
    S = np.array(f["albedo"], F)[None, :] * S
    out = np.zeros((R, 4), F)
    out[:, :3] = S
    assert out.dtype == np.float32
    return {"S": out.reshape(m, m, m, 4), "acc": acc, "V": Vs, "att": atts, "skip": skip, "steps": steps, "m": m}


# ---- the segments -----------------------------------------------------------------------------
def _tanf(x):
    """libm's tanf, the function the library's host code calls for the camera's half angle."""
    fn = ctypes.CDLL("libm.so.6").tanf
    fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
    return F(fn(ctypes.c_float(float(x))))


def pixel_rays(cam, w, h):
    """The caster's primary-ray directions [h, w, 3] (vct_view.h pixel_ray) for a vct.camera.Camera."""
    f, u, r = (np.array(v, F) for v in (cam.front, cam.up, cam.right))
    th = _tanf(F(cam.zoom) * F(0.5) * F(3.14159265358979) / F(180.0))
    aspect = F(w) / F(h)
    x = np.arange(w, dtype=F)[None, :]
    y = np.arange(h, dtype=F)[:, None]
    ndx = np.broadcast_to((F(2.0) * (x + F(0.5)) / F(w) - F(1.0)) * th * aspect, (h, w))
    ndy = np.broadcast_to((F(1.0) - F(2.0) * (y + F(0.5)) / F(h)) * th, (h, w))
    d = np.stack([f[c] + ndx * r[c] + ndy * u[c] for c in range(3)], axis=-1).astype(F)
    il = F(1.0) / np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    out = d * il[..., None]
    assert out.dtype == np.float32
    return out


def origin(n, g0, E, eye):
    return ((np.array(eye, F) - np.array(g0, F)) * (F(n) / F(E))).astype(F)


def rays(n, g0, E, eye, pos4, cam=None):
    """vct_fog_rays_device: -> ray4 [h, w, 4] float32 (d.xyz, len)."""
    pos4 = np.asarray(pos4, F)
    h, w = pos4.shape[:2]
    inv_h = F(n) / F(E)
    o = origin(n, g0, E, eye)
    valid = pos4[..., 3] != 0
    with np.errstate(all="ignore"):
        e = (pos4[..., :3] - np.array(g0, F)) * inv_h
        v = e - o
        ln = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        d = v / ln[..., None]
        ok = valid & (ln > 0) & np.isfinite(ln)
        if cam is not None:
            d = np.where(valid[..., None], d, pixel_rays(cam, w, h))
            ln = np.where(valid, ln, INF)
            ok = ok | ~valid
        ok = ok & np.isfinite(d).all(axis=-1)
    out = np.zeros((h, w, 4), F)
    out[ok, :3] = d[ok]
    out[ok, 3] = ln[ok]
    return out


# ---- the march --------------------------------------------------------------------------------
def slab(n, o, d, ln):
    """The clipped segment of R rays: -> t0, t1 [R] float32 and ok [R] (a segment is left)."""
    nf = F(n)
    with np.errstate(all="ignore"):
        ok = (ln > 0) & np.isfinite(d).all(axis=1)
        t0 = np.zeros(d.shape[0], F)
        t1 = np.where(ok, ln, F(0.0)).astype(F)
        for c in range(3):
            dc = np.where(ok, d[:, c], F(0.0)).astype(F)
            inv = F(1.0) / dc
            clip = ~((dc == 0) | ~np.isfinite(inv))
            inside = (o[c] >= 0) & (o[c] <= nf)
            ok = ok & (clip | inside)
            ta = (F(0.0) - o[c]) * inv
            tb = (nf - o[c]) * inv
            t0 = np.where(clip, np.fmax(t0, np.fmin(ta, tb)), t0).astype(F)
            t1 = np.where(clip, np.fmin(t1, np.fmax(ta, tb)), t1).astype(F)
        null = ~((ln > 0) & np.isfinite(d).all(axis=1))
        ok = ok & (t1 > t0)
    return t0, t1, ok, null


def trilinear(S, level, p):
    """S(p) for R points: S [m, m, m, 4] (z, y, x), p [R, 3] -> [R, 3] float32, and whether a
    corner index was clamped."""
    m = S.shape[0]
    c = p * F(2.0 ** -level) - F(0.5)
    fl = np.floor(c)
    w1 = c - fl
    w = (F(1.0) - w1, w1)
    i0 = fl.astype(np.int64)
    acc = np.zeros((p.shape[0], 3), F)
    clamped = np.zeros(p.shape[0], bool)
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                x, y, z = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
                xc, yc, zc = (np.clip(v, 0, m - 1) for v in (x, y, z))
                clamped |= (xc != x) | (yc != y) | (zc != z)
                wc = (w[dx][:, 0] * w[dy][:, 1]) * w[dz][:, 2]
                acc = fmaf(wc[:, None], S[zc, yc, xc, :3], acc)
    return acc, clamped


def march(n, g0, E, f, eye, ray4, S):
    """vct_fog_march_device: -> dict(fog4 [h, w, 4], steps (int), samples / end / last_len [h, w],
    entered [h, w] (the segment starts inside the grid's box after a clip: t0 > 0),
    clamped [h, w] (a sample used a clamped corner index))."""
    ray4 = np.asarray(ray4, F)
    S = np.asarray(S, F)
    h, w = ray4.shape[:2]
    R = h * w
    r = ray4.reshape(R, 4)
    d, ln = r[:, :3], r[:, 3]
    o = origin(n, g0, E, eye)
    level = int(f["level"])
    sigma = sigma_v(f, n, E)
    ds = F(f["step"]) * F(2.0 ** level)
    t0, t1, ok, null = slab(n, o, d, ln)
    end = np.where(null, END_NULL, np.where(ok, END_SAMPLES, END_EMPTY)).astype(np.int8)
    with np.errstate(all="ignore"):
        t0 = np.where(ok, t0, F(0.0)).astype(F)
        t1 = np.where(ok, t1, F(0.0)).astype(F)
        span = t1 - t0
        N = np.where(ok, np.fmin(np.ceil(span / ds), F(MAX_STEPS)), F(0.0)).astype(np.int64)
        a_full = np.fmin(sigma * ds, F(1.0))
        last_len = np.fmin(span - (N - 1).astype(F) * ds, ds)
        a_last = np.fmin(sigma * last_len, F(1.0))
    T = np.ones(R, F)
    Fc = np.zeros((R, 3), F)
    cnt = np.zeros(R, np.int64)
    clamped = np.zeros(R, bool)
    T_trace = []
    for i in range(int(N.max()) if R else 0):
        act = np.flatnonzero((i < N) & ~(T < T_STOP))
        if not act.size:
            break
        ts = t0[act] + (F(i) + F(0.5)) * ds
        p = o[None, :] + d[act] * ts[:, None]
        Sp, cl = trilinear(S, level, p)
        clamped[act] |= cl
        a = np.where(i == N[act] - 1, a_last[act], a_full).astype(F)
        Ta = T[act] * a
        Fc[act] = fmaf(Ta[:, None], Sp, Fc[act])
        T[act] = T[act] * (F(1.0) - a)
        cnt[act] += 1
        T_trace.append(T.copy())
    end = np.where((end == END_SAMPLES) & (T < T_STOP), END_TSTOP, end).astype(np.int8)
    fog4 = np.concatenate([Fc, T[:, None]], axis=1).astype(F).reshape(h, w, 4)
    return {"fog4": fog4, "steps": int(cnt.sum()), "samples": cnt.reshape(h, w), "end": end.reshape(h, w),
            "last_len": np.where(ok, last_len, F(0.0)).reshape(h, w), "ds": ds, "N": N.reshape(h, w),
            "entered": (ok & (t0 > 0)).reshape(h, w), "clamped": clamped.reshape(h, w), "T_trace": T_trace}


# ---- apply ------------------------------------------------------------------------------------
def apply(fog4, linear4=None):
    """vct_fog_apply_device: -> (linear4 out [h, w, 4] float32, rgba8 [h, w] uint32 by the
    composite's tone curve in float64: the GPU's powf may differ by one step)."""
    fog4 = np.asarray(fog4, F)
    lin = np.zeros_like(fog4) if linear4 is None else np.array(linear4, F, copy=True)

    def tone(v):
        v = v.astype(np.float64)
        v = v / (1.0 + v)
        return np.power(np.where(v < 0, 0.0, v), float(F(0.454545468)))

    with np.errstate(all="ignore"):
        back = lin[..., 3:4] == 0                                    # a composite's background pixel
        display = lin[..., :3].astype(np.float64) * fog4[..., 3:4] + tone(fog4[..., :3])
        lin[..., :3] = fmaf(lin[..., :3], fog4[..., 3:4], fog4[..., :3])
        v = np.where(back, display, tone(lin[..., :3]))
        q = np.clip(np.floor(v * 255.0 + 0.5), 0, 255).astype(np.uint32)
    rgba8 = q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | np.uint32(255 << 24)
    return lin, rgba8.astype(np.uint32)


# ---- the inputs the CPU and GPU tests share -----------------------------------------------------
TAN = 0.1
EYE_IN = (0.1, -0.2, 0.6)          # inside the Cornell box
EYE_OUT = (0.0, 0.0, 4.0)          # outside the grid, looking in (the default camera's side)


def cornell_lights():
    """The sun, a short-range point light (range skips) and a ceiling spot (cone skips)."""
    import vct
    from vct import scenes
    return [vct.directional_light(scenes.LIGHT_DIR, (2.0, 2.0, 1.5)),
            vct.point_light((-0.35, -0.7, 0.45), (1.0, 0.5, 0.2), 0.9),
            vct.spot_light((0.0, 0.95, 0.0), (0.2, -1.0, 0.1), (6.0, 6.0, 5.0), 3.0, cos_inner=0.9397, cos_outer=0.8192)]


_atrium = {}


def atrium(n=32):
    """The atrium at n^3 on the CPU oracle, lit by the sun, computed once: dict(arrays, g0, E,
    grid, level0, lights) with lights = the sun, one point light and one spot light."""
    if n not in _atrium:
        import vct
        from oracle import oracle as O
        from vct import scenes
        O.build()
        arrays = scenes.atrium().arrays()
        g0, E = scenes.grid_for_unit_box(n)
        grid = O.pipeline(n, g0, E, *arrays, scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
        lights = [vct.directional_light(scenes.LIGHT_DIR, (1.5, 1.5, 1.25)),
                  vct.point_light((0.55, -0.3, 0.2), (3.0, 2.0, 1.0), 0.8),
                  vct.spot_light((-0.5, 0.6, 0.0), (0.3, -1.0, 0.2), (5.0, 5.0, 6.0), 2.5, cos_inner=0.94, cos_outer=0.82)]
        for a in (grid["r0"], grid["albedo_occ"], grid["normal"]):
            a.setflags(write=False)
        _atrium[n] = {"arrays": arrays, "g0": g0, "E": E, "grid": grid, "level0": grid["r0"], "lights": lights}
    return _atrium[n]


_alpha = {}


def scene(name, n, aniso=True):
    """-> dict(g0, E, arrays, level0, alpha, lights, inject) of 'cornell' (lights_ref.cornell's
    grid under its light set S) or 'atrium' (under the sun); the alpha pyramid is computed once."""
    if name == "cornell":
        c = lights_ref.cornell(n)
        out = {"g0": c["g0"], "E": c["E"], "arrays": c["arrays"], "level0": c["level0"], "lights": cornell_lights(),
               "inject": lambda ctx: ctx.inject_lights(c["lights"])}
    else:
        from vct import scenes
        c = atrium(n)
        out = {"g0": c["g0"], "E": c["E"], "arrays": c["arrays"], "level0": c["level0"], "lights": c["lights"],
               "inject": lambda ctx: ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)}
    key = (name, n, aniso)
    if key not in _alpha:
        _alpha[key] = shadow_ref.alpha_pyramid(n, out["level0"], aniso)
    out["alpha"] = _alpha[key]
    return out


def eye_rays(n, g0, E, eye, w, h, yaw=-90.0, pitch=0.0):
    """A frame of background rays from `eye` (every pixel's primary ray, len = +inf): the CPU
    tests' stand-in for a G-buffer.  -> (ray4 [h, w, 4], Camera)."""
    from vct.camera import Camera
    cam = Camera(position=eye, yaw=yaw, pitch=pitch)
    return rays(n, g0, E, eye, np.zeros((h, w, 4), F), cam), cam
