"""Reference for include/vct_sky_view.h (TEST INFRASTRUCTURE ONLY).

A numpy float32 restatement of include/vct_spec.h "sky in view", written from that text.  It
composes what the other references already pin: the cone origin and the reflected direction
are spec_ref.Tracer.pixel's (A.5, A.6) vectorised in float32, the cone's alpha is
shadow_ref.march with t_lim = +inf (the receivers grouped by the bit pattern of their
clamped aperture, since a march shares one tau), the transmittance is shadow_ref.visibility,
the sky colour sky_ref.sky_color, the primary rays fog_ref.pixel_rays and the tone curve the
one fog_ref.apply restates.  Everything else is one float32 numpy operation per spec operation.
"""
from __future__ import annotations

import numpy as np

import fog_ref
import shadow_ref
import sky_ref
import spec_ref

F = np.float32
INF = F(np.inf)
R8 = [0.02, 0.05, 0.1, 0.25, 0.5, 1.0, 0.001, 2.5]       # two of them clamp: six distinct tau


def block_roughness(alb, values=R8, shift=0):
    """trace_inputs.block_roughness with the partial blocks at the right and bottom edges
    included (equal to it on a frame of whole 8x8 blocks)."""
    out = np.array(alb, F, copy=True)
    hh, ww = out.shape[:2]
    bw = (ww + 7) // 8
    for by in range((hh + 7) // 8):
        for bx in range(bw):
            out[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8, 3] = values[(by * bw + bx + shift) % len(values)]
    return out


def pixel_roughness(alb, values=R8):
    """A copy of alb with roughness values[(x + 3 y) % len]: every wave holds every aperture."""
    out = np.array(alb, F, copy=True)
    hh, ww = out.shape[:2]
    y, x = np.mgrid[0:hh, 0:ww]
    out[..., 3] = np.array(values, F)[(x + 3 * y) % len(values)]
    return out


def clamp_tau(rough):
    """tau = fminf(fmaxf(roughness, TAU_MIN), TAU_MAX), element-wise (a NaN clamps to TAU_MIN)."""
    return np.fmin(np.fmax(np.asarray(rough, F), F(spec_ref.TAU_MIN)), F(spec_ref.TAU_MAX)).astype(F)


def origins_and_reflections(n, g0, E, P, N, eye):
    """o and r of R receivers: P, N [R, 3] (spec_ref.Tracer.pixel lines 453, 470-475)."""
    P, N = np.asarray(P, F), np.asarray(N, F)
    inv_h = F(n) / F(E)
    e = np.array(eye, F)
    with np.errstate(all="ignore"):
        o = (P - np.array(g0, F)[None, :]) * inv_h + N
        v = e[None, :] - P
        vl = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        v = v / vl[:, None]
        ndv = (N[:, 0] * v[:, 0] + N[:, 1] * v[:, 1]) + N[:, 2] * v[:, 2]
        k2 = F(2.0) * ndv
        r = k2[:, None] * N - v
    assert o.dtype == np.float32 and r.dtype == np.float32
    return o, r


def receivers(n, g0, E, alpha, aniso, P, N, rough, eye, sky):
    """-> dict(s [R, 4] (S.rgb, T), a, T, steps, end [R], r [R, 3], tau [R])."""
    R = np.asarray(P).shape[0]
    o, r = origins_and_reflections(n, g0, E, P, N, eye)
    tau = clamp_tau(rough)
    a = np.zeros(R, F)
    steps = np.zeros(R, np.int64)
    end = np.zeros(R, np.int8)
    with np.errstate(all="ignore"):
        for bits in np.unique(tau.view(np.uint32)):
            k = np.flatnonzero(tau.view(np.uint32) == bits)
            a[k], steps[k], end[k] = shadow_ref.march(alpha, n, aniso, o[k], r[k], np.full(k.size, INF, F),
                                                      float(np.uint32(bits).view(F)))
        T = shadow_ref.visibility(a)
        S = T[:, None] * sky_ref.sky_color(r, sky)
    return {"s": np.concatenate([S, T[:, None]], axis=1).astype(F), "a": a, "T": T, "steps": steps, "end": end,
            "r": r, "tau": tau}


def frame(n, g0, E, alpha, aniso, pos4, nrm4, alb4, eye, sky, specular=True):
    """vct_sky_specular_device: -> dict(skyspec4 [h, w, 4], steps (int), steps_px [h, w], rec, px: (y, x))."""
    pos4, nrm4, alb4 = (np.asarray(a, F) for a in (pos4, nrm4, alb4))
    h, w = pos4.shape[:2]
    fy, fx = np.nonzero(pos4[..., 3] != 0)
    out = np.zeros((h, w, 4), F)
    steps_px = np.zeros((h, w), np.int64)
    if not specular:
        return {"skyspec4": out, "steps": 0, "steps_px": steps_px, "rec": None, "px": (fy, fx)}
    rec = receivers(n, g0, E, alpha, aniso, pos4[fy, fx, :3], nrm4[fy, fx, :3], alb4[fy, fx, 3], eye, sky)
    out[fy, fx] = rec["s"]
    steps_px[fy, fx] = rec["steps"]
    return {"skyspec4": out, "steps": int(rec["steps"].sum()), "steps_px": steps_px, "rec": rec, "px": (fy, fx)}


def add_to_spec(spec4, pos4, skyspec4):
    """spec.rgb + S.rgb at the valid pixels, alpha and the background untouched."""
    out = np.array(spec4, F, copy=True)
    valid = np.asarray(pos4, F)[..., 3] != 0
    with np.errstate(all="ignore"):
        out[valid, :3] = out[valid, :3] + np.asarray(skyspec4, F)[valid, :3]
    return out


def coverage(rec):
    """Shares over the valid pixels: alpha stop; left the grid with 0 < T < 1; left with T = 1."""
    end, T = rec["end"], rec["T"]
    m = max(end.size, 1)
    left = end == shadow_ref.END_LEFT
    return {"valid": int(end.size), "alpha stop": float((end == shadow_ref.END_ALPHA).sum()) / m,
            "left partial": float((left & (T > 0) & (T < 1)).sum()) / m,
            "left clear": float((left & (T == 1)).sum()) / m,
            "taus": int(np.unique(rec["tau"].view(np.uint32)).size), "longest": int(rec["steps"].max(initial=0))}


def tone8(c):
    """The composite's present step on [..., 3] float32 -> [...] packed uint32, alpha 255, by the
    tone curve in float64 as fog_ref.apply restates it (the GPU's powf may differ by one step)."""
    v = np.asarray(c, F).astype(np.float64)
    with np.errstate(all="ignore"):
        v = v / (1.0 + v)
        v = np.power(np.where(v < 0, 0.0, v), float(F(0.454545468)))
        q = np.clip(np.floor(v * 255.0 + 0.5), 0, 255).astype(np.uint32)
    return (q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | np.uint32(255 << 24)).astype(np.uint32)


def background(cam, pos4, sky, linear4=None, rgba8=None):
    """vct_sky_background_device: -> (linear4 out [h, w, 4] float32, rgba8 out [h, w] uint32);
    the inputs (default: zeros) pass through at the valid pixels."""
    pos4 = np.asarray(pos4, F)
    h, w = pos4.shape[:2]
    lin = np.zeros((h, w, 4), F) if linear4 is None else np.array(linear4, F, copy=True)
    q = np.zeros((h, w), np.uint32) if rgba8 is None else np.array(rgba8, np.uint32, copy=True)
    bg = pos4[..., 3] == 0
    c = sky_ref.sky_color(fog_ref.pixel_rays(cam, w, h), sky)
    lin[bg, :3] = c[bg]
    lin[bg, 3] = 1.0
    q[bg] = tone8(c)[bg]
    return lin, q


def bytes_within_one(a, b):
    """Two packed RGBA8 frames differ by at most one step in every channel."""
    a, b = (np.ascontiguousarray(v, np.uint32).view(np.uint8).astype(np.int16) for v in (a, b))
    return bool((np.abs(a - b) <= 1).all())
