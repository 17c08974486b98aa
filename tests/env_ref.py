"""Reference for include/vct_env.h (TEST INFRASTRUCTURE ONLY).

A numpy float32 restatement of include/vct_spec.h "environment sky", written from that text:
the box mips, the input rules, and Env(d, tau) step by step, one float32 numpy operation per
spec operation with the fused ones through shadow_ref.fmaf.  Everything but the colour is what
the other references already pin: the diffuse receivers, cones, a_k and T_k are sky_ref's, the
specular cone sky_view_ref's, the primary rays fog_ref.pixel_rays and the tone curve
sky_view_ref.tone8.  lookup64 evaluates the same formulas in float64 (no rounding rule) for the
tolerance tests.

An env record is a dict(frame [3][3], scale); a pyramid is the list of levels mips() returns.
"""
from __future__ import annotations

import numpy as np

import fog_ref
import sky_ref
import sky_view_ref
import spec_ref
from shadow_ref import fmaf

F = np.float32
MAX_DIM = 2048
TEXEL_LIMIT = F(2.0 ** 52)            # VCT_ENV_TEXEL_LIMIT (include/vct_spec.h)
ORTHO_EPS = 2.0 ** -20                # VCT_GBUF_ORTHO_EPS
IDENTITY = {"frame": ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), "scale": 1.0}
# the map's +z is the world's +y (a 90 degree frame): rows are the world directions of map x, y, z
Y_UP = {"frame": ((1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)), "scale": 1.0}


def tilted(scale=3.7, yaw=0.7, pitch=-0.4, roll=0.3):
    """An orthonormal frame with no zero entry (float64 rotations, rounded to float32)."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    m = (rz @ rx @ ry).astype(F)
    return {"frame": tuple(tuple(float(v) for v in row) for row in m), "scale": scale}


# ---- the input rules -----------------------------------------------------------------------------
def size_error(size):
    if size < 1 or size > MAX_DIM or size & (size - 1):
        return "size must be a power of two in 1..VCT_ENV_MAX_DIM"
    return None


def map_error(level0):
    """The texel rule of vct_set_env on [S, S, 4] float32: None, or what is wrong."""
    m = np.asarray(level0, F)
    if m.ndim != 3 or m.shape[0] != m.shape[1] or m.shape[2] != 4:
        return "shape"
    if size_error(m.shape[0]):
        return size_error(m.shape[0])
    rgb = m[..., :3]
    if not np.isfinite(rgb).all():
        return "non-finite texel"
    if np.signbit(rgb).any():
        return "negative texel"
    if (rgb > TEXEL_LIMIT).any():
        return "texel above VCT_ENV_TEXEL_LIMIT"
    return None


def record_error(env):
    """The record rule: None, or what is wrong."""
    fr = np.array(env["frame"], F)
    if fr.shape != (3, 3) or not np.isfinite(fr).all():
        return "non-finite frame"
    f64 = fr.astype(np.float64)
    for i in range(3):
        for j in range(i, 3):
            g = (f64[i, 0] * f64[j, 0] + f64[i, 1] * f64[j, 1]) + f64[i, 2] * f64[j, 2]
            if not abs(g - (1.0 if i == j else 0.0)) <= ORTHO_EPS:
                return "frame rows not orthonormal"
    s = F(env["scale"])
    if not np.isfinite(s):
        return "non-finite scale"
    if np.signbit(s):
        return "negative scale"
    if s > TEXEL_LIMIT:
        return "scale above VCT_ENV_TEXEL_LIMIT"
    return None


# ---- the pyramid -----------------------------------------------------------------------------------
def mips(level0):
    """[S, S, 4] -> the levels j = 0 .. lg S, each [S_j, S_j, 4] float32 (row y, column x)."""
    lv = [np.ascontiguousarray(level0, F)]
    assert map_error(lv[0]) is None, map_error(lv[0])
    with np.errstate(all="ignore"):
        while lv[-1].shape[0] > 1:
            m = lv[-1]
            a00, a10, a01, a11 = m[0::2, 0::2], m[0::2, 1::2], m[1::2, 0::2], m[1::2, 1::2]
            lv.append((((a00 + a10) + (a01 + a11)) * F(0.25)).astype(F))
    return lv


# ---- Env(d, tau) -----------------------------------------------------------------------------------
def log2_f32(x):
    """A.6's spec_log2 on an array of float32 >= 1 (spec_ref.log2 vectorised)."""
    x = np.ascontiguousarray(x, F)
    bits = x.view(np.uint32)
    e = ((bits >> 23) & 0xFF).astype(np.int32) - 127
    f = ((bits & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(F)
    big = f > F(spec_ref.LOG2_SQRT2)
    f = np.where(big, f * F(0.5), f).astype(F)
    e = e + big
    s = (f - F(1.0)) / (f + F(1.0))
    z = s * s
    p = np.full(x.shape, F(spec_ref.C9), F)
    for c in (spec_ref.C7, spec_ref.C5, spec_ref.C3, 1.0):
        p = fmaf(p, z, F(c))
    ln = (F(2.0) * s) * p
    return fmaf(ln, F(spec_ref.INV_LN2), e.astype(F))


def dot3(a, d):
    return (a[0] * d[..., 0] + a[1] * d[..., 1]) + a[2] * d[..., 2]


def oct_point(env, d):
    """Steps 1 and 2: d [N, 3] -> (p [N, 2] float32, ok [N]); p is (0, 0) where not ok."""
    d = np.asarray(d, F)
    fr = np.array(env["frame"], F)
    with np.errstate(all="ignore"):
        e = np.stack([dot3(fr[c], d) for c in range(3)], axis=-1)
        s = (np.abs(e[..., 0]) + np.abs(e[..., 1])) + np.abs(e[..., 2])
        ok = (s > 0) & (s < np.inf)
        px, py = e[..., 0] / s, e[..., 1] / s
        one = F(1.0)
        qx = (one - np.abs(py)) * np.copysign(one, px)
        qy = (one - np.abs(px)) * np.copysign(one, py)
        fold = e[..., 2] < 0
        px, py = np.where(fold, qx, px), np.where(fold, qy, py)
    p = np.stack([np.where(ok, px, F(0)), np.where(ok, py, F(0))], axis=-1).astype(F)
    return p, ok


def level_of(tau, S):
    """Step 3: tau [N] -> (m float32, j0 int, fr float32)."""
    lg = int(S).bit_length() - 1
    tau = np.asarray(tau, F)
    with np.errstate(all="ignore"):
        x = np.fmin(np.fmax(tau * F(S), F(1.0)), F(S)).astype(F)
        m = np.fmin(log2_f32(x), F(lg)).astype(F)
    j0 = m.astype(np.int32)
    return m, j0, (m - j0.astype(F)).astype(F)


def taps(Sj, p, dtype=F):
    """Step 4's addressing at a level of Sj texels: p [N, 2] -> (rows [4, N], cols [4, N], fu, fv)
    for the taps a, b, c, d, fold rule applied."""
    T = dtype
    p = np.asarray(p, T)
    u = (p[:, 0] * T(0.5) + T(0.5)) * T(Sj) - T(0.5)
    v = (p[:, 1] * T(0.5) + T(0.5)) * T(Sj) - T(0.5)
    fi, fk = np.floor(u), np.floor(v)
    fu, fv = (u - fi).astype(T), (v - fk).astype(T)
    i0, k0 = fi.astype(np.int64), fk.astype(np.int64)
    rows, cols = [], []
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = i0 + dx, k0 + dy
            xc, yc = np.clip(x, 0, Sj - 1), np.clip(y, 0, Sj - 1)
            rows.append(np.where(x == xc, yc, Sj - 1 - yc))
            cols.append(np.where(y == yc, xc, Sj - 1 - xc))
    return np.array(rows), np.array(cols), fu, fv


def bilinear(level, p):
    """Step 4: B_j at p [N, 2] -> [N, 3] float32."""
    lv = np.asarray(level, F)
    rows, cols, fu, fv = taps(lv.shape[0], p)
    a, b, c, d = (lv[rows[k], cols[k], :3] for k in range(4))
    fu, fv = fu[:, None], fv[:, None]
    t0 = fmaf(fu, b - a, a)
    t1 = fmaf(fu, d - c, c)
    return fmaf(fv, t1 - t0, t0)


def lookup(pyr, env, d, tau):
    """Env(d, tau): d [N, 3], tau [N] or a scalar -> (rgb [N, 3] float32, m [N] float32)."""
    d = np.asarray(d, F).reshape(-1, 3)
    tau = np.broadcast_to(np.asarray(tau, F), d.shape[:1])
    S = pyr[0].shape[0]
    lg = len(pyr) - 1
    p, ok = oct_point(env, d)
    m, j0, fr = level_of(tau, S)
    j0 = np.where(ok, j0, lg)
    fr = np.where(ok, fr, F(0)).astype(F)
    E = np.zeros((d.shape[0], 3), F)
    for j in range(lg + 1):
        k = np.flatnonzero(j0 == j)
        if not k.size:
            continue
        B0 = bilinear(pyr[j], p[k])
        two = (fr[k] > 0) & (j < lg)
        out = B0.copy()
        if two.any():
            B1 = bilinear(pyr[j + 1], p[k][two])
            out[two] = fmaf(fr[k][two][:, None], B1 - B0[two], B0[two])
        E[k] = out
    with np.errstate(all="ignore"):
        rgb = (E * F(env["scale"])).astype(F)
    return rgb, m


def lookup64(pyr, env, d, tau):
    """The same formulas evaluated in float64 from the float32 inputs (the exact log2 in step 3
    is replaced by the float32 level, so both take the same level pair): [N, 3] float64."""
    d = np.asarray(d, F).reshape(-1, 3).astype(np.float64)
    tau = np.broadcast_to(np.asarray(tau, F), d.shape[:1])
    fr3 = np.array(env["frame"], F).astype(np.float64)
    S, lg = pyr[0].shape[0], len(pyr) - 1
    e = d @ fr3.T
    s = np.abs(e).sum(axis=1)
    p = e[:, :2] / s[:, None]
    q = (1.0 - np.abs(p[:, ::-1])) * np.copysign(1.0, p)
    p = np.where((e[:, 2] < 0)[:, None], q, p)
    _, j0, fr = level_of(tau, S)

    def bil(j, pp):
        lv = pyr[j].astype(np.float64)
        rows, cols, fu, fv = taps(lv.shape[0], pp, np.float64)
        a, b, c, dd = (lv[rows[k], cols[k], :3] for k in range(4))
        t0 = a + fu[:, None] * (b - a)
        t1 = c + fu[:, None] * (dd - c)
        return t0 + fv[:, None] * (t1 - t0)

    E = np.zeros((d.shape[0], 3))
    for j in range(lg + 1):
        k = np.flatnonzero(j0 == j)
        if k.size:
            B0 = bil(j, p[k])
            B1 = bil(min(j + 1, lg), p[k])
            E[k] = B0 + fr[k].astype(np.float64)[:, None] * (B1 - B0)
    return E * float(F(env["scale"]))


# ---- directions of the map (float64; convenience, as vct.env's helpers) ------------------------------
def oct_decode(p):
    """p [..., 2] in [-1, 1]^2 -> unit map-space directions [..., 3] (float64)."""
    p = np.asarray(p, np.float64)
    z = 1.0 - np.abs(p[..., 0]) - np.abs(p[..., 1])
    x = np.where(z < 0, (1.0 - np.abs(p[..., 1])) * np.copysign(1.0, p[..., 0]), p[..., 0])
    y = np.where(z < 0, (1.0 - np.abs(p[..., 0])) * np.copysign(1.0, p[..., 1]), p[..., 1])
    e = np.stack([x, y, z], axis=-1)
    return e / np.linalg.norm(e, axis=-1, keepdims=True)


def texel_dirs(S):
    """Map-space unit directions of the S x S texel centres, [S, S, 3] float64 (row y, column x)."""
    c = (np.arange(S) + 0.5) * 2.0 / S - 1.0
    return oct_decode(np.stack(np.meshgrid(c, c, indexing="xy"), axis=-1))


def world_dirs(env, e):
    """Map-space directions -> world (frame is orthonormal: d = frame^T e)."""
    return np.asarray(e, np.float64) @ np.array(env["frame"], F).astype(np.float64)


# ---- the four calls ------------------------------------------------------------------------------------
def _accumulate(rec, rows, col):
    """'sky light''s per-receiver sum with the colours col [R, K, 3]."""
    R, K = rec["T"].shape
    acc = np.zeros((R, 3), F)
    vis = np.zeros(R, F)
    with np.errstate(all="ignore"):
        for k in range(K):
            w = rows[k, 3]
            acc = fmaf((w * rec["T"][:, k])[:, None], col[:, k], acc)
            vis = fmaf(w, rec["T"][:, k], vis)
    return np.concatenate([acc, vis[:, None]], axis=1).astype(F)


def receivers(rec, pyr, env, n_diffuse):
    """Sk [R, 4] of a sky_ref.receivers() dict (its T and d), with Env for Sky."""
    rows, tau = sky_ref.cone_set(n_diffuse)
    R, K = rec["T"].shape
    col, _ = lookup(pyr, env, rec["d"].reshape(-1, 3), F(tau))
    return _accumulate(rec, rows, col.reshape(R, K, 3))


def frame(n, g0, E, alpha, aniso, pos4, nrm4, pyr, env, n_diffuse=9, base=None):
    """vct_env_cones_device: -> dict(sky4 [h, w, 4], steps).  base: sky_ref.frame's dict of the
    same records (any sky: only its T, d and steps are read), computed here when None."""
    if base is None:
        base = sky_ref.frame(n, g0, E, alpha, aniso, pos4, nrm4, sky_ref.SKY_ZERO, n_diffuse)
    sky4 = np.zeros_like(base["sky4"])
    if n_diffuse:
        sky4[base["px"]] = receivers(base["rec"], pyr, env, n_diffuse)
    return {"sky4": sky4, "steps": base["steps"], "rec": base["rec"], "px": base["px"]}


def inject(n, g0, E, ao, nm, level0, alpha, aniso, pyr, env, n_diffuse=9):
    """vct_inject_env: level 0 with L.rgb + A.rgb * Sk.rgb at every bounce source."""
    import bounce_ref
    (pos, nrm, alb), (z, y, x) = bounce_ref.source_gbuffer(n, g0, E, ao, nm)
    rec = sky_ref.receivers(n, g0, E, alpha, aniso, pos[0, :, :3], nrm[0, :, :3], sky_ref.SKY_ZERO, n_diffuse)
    out = np.array(level0, F, copy=True)
    if n_diffuse:
        sk = receivers(rec, pyr, env, n_diffuse)
        prod = alb[0, :, :3] * sk[:, :3]
        out[z, y, x, :3] = out[z, y, x, :3] + prod
    return out


def specular(n, g0, E, alpha, aniso, pos4, nrm4, alb4, eye, pyr, env, specular=True, base=None):
    """vct_env_specular_device: -> dict(skyspec4 [h, w, 4], steps).  base: sky_view_ref.frame's
    dict of the same records (its T, r, tau and steps are read), computed here when None."""
    if base is None:
        base = sky_view_ref.frame(n, g0, E, alpha, aniso, pos4, nrm4, alb4, eye, sky_ref.SKY_ZERO, specular)
    out = np.zeros_like(base["skyspec4"])
    if specular and base["rec"] is not None:
        rec = base["rec"]
        col, _ = lookup(pyr, env, rec["r"], rec["tau"])
        with np.errstate(all="ignore"):
            S = rec["T"][:, None] * col
        out[base["px"]] = np.concatenate([S, rec["T"][:, None]], axis=1).astype(F)
    return {"skyspec4": out, "steps": base["steps"], "rec": base["rec"], "px": base["px"]}


def background(cam, pos4, pyr, env, linear4=None, rgba8=None):
    """vct_env_background_device: -> (linear4 out, rgba8 out), as sky_view_ref.background."""
    pos4 = np.asarray(pos4, F)
    h, w = pos4.shape[:2]
    lin = np.zeros((h, w, 4), F) if linear4 is None else np.array(linear4, F, copy=True)
    q = np.zeros((h, w), np.uint32) if rgba8 is None else np.array(rgba8, np.uint32, copy=True)
    bg = pos4[..., 3] == 0
    c, _ = lookup(pyr, env, fog_ref.pixel_rays(cam, w, h).reshape(-1, 3), F(0.0))
    c = c.reshape(h, w, 3)
    lin[bg, :3] = c[bg]
    lin[bg, 3] = 1.0
    q[bg] = sky_view_ref.tone8(c)[bg]
    return lin, q


def constant_sky(c):
    """The vct_sky whose three colours are c (the identity tests' counterpart)."""
    c = tuple(float(v) for v in c)
    return {"up": (0.0, 1.0, 0.0), "zenith": c, "horizon": c, "ground": c}


def constant_map(S, c, alpha=1.0):
    m = np.empty((S, S, 4), F)
    m[..., :3] = np.array(c, F)
    m[..., 3] = alpha
    return m


def random_map(S, seed=0):
    return np.random.default_rng(seed).random((S, S, 4), dtype=np.float32)


def sun_map(S=64, seed=1, at=(41, 13), value=4096.0):
    """A dim random map with one bright texel."""
    m = (random_map(S, seed) * F(0.125)).astype(F)
    m[at[1], at[0], :3] = (value, value * 0.75, value * 0.5)
    return m


def to_ctypes(env):
    import vct
    return vct.env_sky(env["frame"], env["scale"])
