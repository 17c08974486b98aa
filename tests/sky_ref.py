"""Reference for include/vct_sky.h (TEST INFRASTRUCTURE ONLY).

A numpy float32 restatement of include/vct_spec.h "sky light", written from that text.  It
composes what the other references already pin: the cone origin and tangent frame are
spec_ref.Tracer.pixel's (A.5) vectorised in float32, the cone rows are the header's, and each
cone's alpha is shadow_ref.march with t_lim = +inf and the diffuse aperture, which is the
alpha of A.6's march bit for bit (tests/test_shadow.py).  The fused operations go through
shadow_ref.fmaf; everything else is one float32 numpy operation per spec operation.

A sky is a dict(up, zenith, horizon, ground) of three floats each.
"""
from __future__ import annotations

import numpy as np

import bounce_ref
import shadow_ref
import spec_ref
from shadow_ref import fmaf

F = np.float32
INF = F(np.inf)

# include/vct_spec.h VCT_CONES16 (spec_ref has the 1- and 9-cone rows only)
_C30, _W30, _W60 = 0.866025388, 0.0838349238, 0.0484021157
CONES16 = [(1.0, 0.0, 0.0, 0.0968042314),
           (_C30, 0.5, 0.0, _W30), (_C30, 0.154508501, 0.475528270, _W30), (_C30, -0.404508501, 0.293892622, _W30),
           (_C30, -0.404508501, -0.293892622, _W30), (_C30, 0.154508501, -0.475528270, _W30),
           (0.5, 0.823639095, 0.267616570, _W60), (0.5, 0.509036958, 0.700629294, _W60),
           (0.5, 0.0, 0.866025388, _W60), (0.5, -0.509036958, 0.700629294, _W60),
           (0.5, -0.823639095, 0.267616570, _W60), (0.5, -0.823639095, -0.267616570, _W60),
           (0.5, -0.509036958, -0.700629294, _W60), (0.5, 0.0, -0.866025388, _W60),
           (0.5, 0.509036958, -0.700629294, _W60), (0.5, 0.823639095, -0.267616570, _W60)]

SKY = {"up": (0.0, 1.0, 0.0), "zenith": (0.25, 0.5, 1.0), "horizon": (0.75, 0.625, 0.5), "ground": (0.125, 0.0625, 0.03125)}
# no exact products: a tilted, un-normalised up and colours that are not dyadic
SKY_TILTED = {"up": (0.3, 2.0, -0.4), "zenith": (0.21, 0.47, 0.93), "horizon": (0.71, 0.63, 0.52),
              "ground": (0.11, 0.07, 0.03)}
SKY_ZERO = {"up": (0.0, 1.0, 0.0), "zenith": (0.0, 0.0, 0.0), "horizon": (0.0, 0.0, 0.0), "ground": (0.0, 0.0, 0.0)}
END_NAMES = shadow_ref.END_NAMES


def cone_set(n_diffuse):
    """-> (rows [K, 4] float32 (cn, ct, cb, w), tau) of the context's diffuse cone set."""
    rows = {0: [], 1: spec_ref.CONES1, 9: spec_ref.CONES9, 16: CONES16}[n_diffuse]
    tau = spec_ref.TAN20 if n_diffuse == 16 else spec_ref.TAN30
    return np.array(rows, F).reshape(-1, 4), float(tau)


def up_n(up):
    """`up` normalised as vct_inject_directional normalises its direction (float32 throughout)."""
    u = np.array(up, F)
    with np.errstate(all="ignore"):
        ln = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
        return (u / ln).astype(F)


def sky_color(d, sky):
    """Sky(d) for directions d [..., 3] -> [..., 3] float32; branch-free, no fused operation."""
    d = np.asarray(d, F)
    un = up_n(sky["up"])
    z, h, g = (np.array(sky[k], F) for k in ("zenith", "horizon", "ground"))
    with np.errstate(all="ignore"):
        u = (d[..., 0] * un[0] + d[..., 1] * un[1]) + d[..., 2] * un[2]
        s_up = np.fmin(np.fmax(u, F(0.0)), F(1.0))[..., None]
        s_dn = np.fmin(np.fmax(-u, F(0.0)), F(1.0))[..., None]
        out = (h + (z - h) * s_up) + (g - h) * s_dn
    assert out.dtype == np.float32
    return out


def origins_and_directions(n, g0, E, P, N, rows):
    """A.5 for R receivers: P, N [R, 3] -> o [R, 3], d [R, K, 3] (spec_ref.Tracer.pixel's operations)."""
    P, N = np.asarray(P, F), np.asarray(N, F)
    inv_h = F(n) / F(E)
    with np.errstate(all="ignore"):
        o = (P - np.array(g0, F)[None, :]) * inv_h + N
        nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
        sgn = np.copysign(F(1.0), nz)
        ka = F(-1.0) / (sgn + nz)
        kb = (nx * ny) * ka
        T = np.stack([F(1.0) + ((sgn * nx) * nx) * ka, sgn * kb, -(sgn * nx)], axis=1)
        B = np.stack([kb, sgn + (ny * ny) * ka, -ny], axis=1)
        cn, ct, cb = (rows[:, k][None, :, None] for k in range(3))
        d = (cn * N[:, None, :] + ct * T[:, None, :]) + cb * B[:, None, :]
    assert o.dtype == np.float32 and d.dtype == np.float32
    return o, d


def receivers(n, g0, E, alpha, aniso, P, N, sky, n_diffuse):
    """The sky of R receivers: -> dict(sk [R, 4] (Sk.rgb, vis), a, T, steps, end [R, K], d)."""
    rows, tau = cone_set(n_diffuse)
    R, K = np.asarray(P).shape[0], rows.shape[0]
    o, d = origins_and_directions(n, g0, E, P, N, rows)
    a = np.zeros((R, K), F)
    steps = np.zeros((R, K), np.int64)
    end = np.zeros((R, K), np.int8)
    acc = np.zeros((R, 3), F)
    vis = np.zeros(R, F)
    with np.errstate(all="ignore"):
        for k in range(K):
            a[:, k], steps[:, k], end[:, k] = shadow_ref.march(alpha, n, aniso, o, d[:, k], np.full(R, INF, F), tau)
        T = shadow_ref.visibility(a)
        col = sky_color(d, sky)
        for k in range(K):                                            # set order
            w = rows[k, 3]
            acc = fmaf((w * T[:, k])[:, None], col[:, k], acc)
            vis = fmaf(w, T[:, k], vis)
    return {"sk": np.concatenate([acc, vis[:, None]], axis=1).astype(F), "a": a, "T": T, "steps": steps, "end": end,
            "d": d}


def frame(n, g0, E, alpha, aniso, pos4, nrm4, sky, n_diffuse=9):
    """vct_sky_cones_device: -> dict(sky4 [h, w, 4], steps (int), rec: receivers()' dict, px: (y, x))."""
    pos4, nrm4 = np.asarray(pos4, F), np.asarray(nrm4, F)
    h, w = pos4.shape[:2]
    fy, fx = np.nonzero(pos4[..., 3] != 0)
    rec = receivers(n, g0, E, alpha, aniso, pos4[fy, fx, :3], nrm4[fy, fx, :3], sky, n_diffuse)
    sky4 = np.zeros((h, w, 4), F)
    if n_diffuse:
        sky4[fy, fx] = rec["sk"]
    return {"sky4": sky4, "steps": int(rec["steps"].sum()), "rec": rec, "px": (fy, fx)}


def add_to_diffuse(diffuse4, pos4, sky4):
    """diffuse.rgb + sky.rgb at the valid pixels, alpha and the background untouched."""
    out = np.array(diffuse4, F, copy=True)
    valid = np.asarray(pos4, F)[..., 3] != 0
    out[valid, :3] = out[valid, :3] + np.asarray(sky4, F)[valid, :3]
    return out


def inject(n, g0, E, ao, nm, level0, alpha, aniso, sky, n_diffuse=9):
    """vct_inject_sky: -> (level 0 with L.rgb + A.rgb * Sk.rgb at every bounce source, receivers()' dict)."""
    (pos, nrm, alb), (z, y, x) = bounce_ref.source_gbuffer(n, g0, E, ao, nm)
    rec = receivers(n, g0, E, alpha, aniso, pos[0, :, :3], nrm[0, :, :3], sky, n_diffuse)
    out = np.array(level0, F, copy=True)
    if n_diffuse:
        prod = alb[0, :, :3] * rec["sk"][:, :3]
        out[z, y, x, :3] = out[z, y, x, :3] + prod                    # float32: one multiply, one add
    assert out.dtype == np.float32
    return out, rec


def coverage(rec):
    """Shares over the cones of a receivers() dict: alpha stop; left the grid with 0 < T < 1."""
    end, T = rec["end"], rec["T"]
    m = max(end.size, 1)
    return {"cones": int(end.size), "alpha stop": float((end == shadow_ref.END_ALPHA).sum()) / m,
            "left partial": float(((end == shadow_ref.END_LEFT) & (T > 0) & (T < 1)).sum()) / m,
            "left clear": float(((end == shadow_ref.END_LEFT) & (T == 1)).sum()) / m,
            "lit receivers": float((rec["sk"][:, 3] > 0).mean()) if rec["sk"].shape[0] else 0.0}


def to_ctypes(sky):
    import vct
    return vct.sky_light(sky["zenith"], sky["horizon"], sky["ground"], sky["up"])
