"""Reference for include/vct_query.h (TEST INFRASTRUCTURE ONLY).

A vectorised numpy float32 restatement of include/vct_spec.h "cone queries" and "probe grid",
written from that text: every cone advances through its own march (its own t, D, l0, fr: the
aperture is per cone), one step per iteration over the cones that still march, and everything
per cone is one float32 numpy operation in the order the spec gives.  The fused operations go
through shadow_ref.fmaf, an exact vectorised binary32 fma; the log2 is the spec's polynomial in
float32.  It does not import the library; the pyramid it samples is the CPU oracle's.

A cone list is a float32 array [R, 12]: the vct_cone records (p, tau, d, t_lim, off, valid).
A probe grid is a dict(origin (3 floats), spacing, dims (dx, dy, dz)).
"""
from __future__ import annotations

import numpy as np

import lights_ref
import sky_ref
import sky_view_ref
import spec_ref
from shadow_ref import fmaf

F = np.float32
INF = F(np.inf)
NAN = F(np.nan)
MAX_STEPS = 4096                                   # VCT_QUERY_MAX_STEPS
PROBE_MAX_DIM = 256                                # VCT_PROBE_MAX_DIM
ALPHA_STOP = F(spec_ref.ALPHA_STOP)
TAU_MIN, TAU_MAX = F(spec_ref.TAU_MIN), F(spec_ref.TAU_MAX)
END_SKIPPED, END_ALPHA, END_LEFT, END_LIMIT, END_CAP = -1, 0, 1, 2, 3      # how a cone ended
END_NAMES = {END_ALPHA: "alpha stop", END_LEFT: "left the grid", END_LIMIT: "t_lim"}


def log2(x):
    """The spec's log2 (vct_spec.h VCT_LOG2_*) of float32 x >= 1, element-wise in float32."""
    x = np.ascontiguousarray(x, F)
    bits = x.view(np.uint32)
    e = ((bits >> np.uint32(23)) & np.uint32(0xFF)).astype(np.int32) - 127
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


# ---- the pyramid ------------------------------------------------------------------------------
def pyramid(n, level0, aniso=True):
    """{level: [n_l, n_l, n_l, 4] volumes (z, y, x), one per face} of the pyramid K3 builds from
    `level0` (the CPU oracle's build), level 0 included."""
    from oracle import oracle as O
    O.build()
    level0 = np.ascontiguousarray(level0, F)
    out = {0: [level0]}
    for l, vols in O.pyramid_levels(n, O.build_mips(n, level0, aniso), aniso).items():
        out[l] = [np.ascontiguousarray(v) for v in vols]
    return out


_pyr = {}


def cornell_pyramid(n, aniso=True):
    """The pyramid of lights_ref.cornell(n)'s level 0, computed once."""
    if (n, aniso) not in _pyr:
        _pyr[(n, aniso)] = pyramid(n, lights_ref.cornell(n)["level0"], aniso)
    return _pyr[(n, aniso)]


# ---- cone lists -------------------------------------------------------------------------------
def make_cones(p, d, tau, t_lim=INF, off=0.0, valid=1.0):
    """-> [R, 12] float32 records; every argument broadcasts against p [R, 3]."""
    p = np.asarray(p, F).reshape(-1, 3)
    R = p.shape[0]
    out = np.empty((R, 12), F)
    out[:, 0:3] = p
    out[:, 3] = np.broadcast_to(np.asarray(tau, F), (R,))
    out[:, 4:7] = np.broadcast_to(np.asarray(d, F), (R, 3))
    out[:, 7] = np.broadcast_to(np.asarray(t_lim, F), (R,))
    out[:, 8:11] = np.broadcast_to(np.asarray(off, F), (R, 3))
    out[:, 11] = np.broadcast_to(np.asarray(valid, F), (R,))
    return out


def specular_cones(n, g0, E, pos4, nrm4, alb4, eye):
    """The specular-identity cones of a frame, one per pixel in row order: p = P, off = N, d = the
    reflected direction, tau = alb.w, t_lim = +inf, valid = pos.w."""
    pos4, nrm4, alb4 = (np.asarray(a, F).reshape(-1, 4) for a in (pos4, nrm4, alb4))
    _, r = sky_view_ref.origins_and_reflections(n, g0, E, pos4[:, :3], nrm4[:, :3], eye)
    return make_cones(pos4[:, :3], r, alb4[:, 3], INF, nrm4[:, :3], pos4[:, 3])


def diffuse_cones(n, g0, E, pos4, nrm4, n_diffuse):
    """The diffuse-identity cones of a frame, pixel-major, K per pixel in set order; -> (cones
    [R * K, 12], rows [K, 4])."""
    pos4, nrm4 = (np.asarray(a, F).reshape(-1, 4) for a in (pos4, nrm4))
    rows, tau = sky_ref.cone_set(n_diffuse)
    K = rows.shape[0]
    _, d = sky_ref.origins_and_directions(n, g0, E, pos4[:, :3], nrm4[:, :3], rows)
    rep = lambda a: np.repeat(a, K, axis=0)
    return make_cones(rep(pos4[:, :3]), d.reshape(-1, 3), F(tau), INF, rep(nrm4[:, :3]), rep(pos4[:, 3])), rows


def accumulate_diffuse(out4, rows):
    """diffuse4 [R, 4] from the query results [R * K, 4] of diffuse_cones: irr = fmaf(w, c, irr),
    occ = fmaf(w, a, occ) in row order, (irr, 1 - occ)."""
    K = rows.shape[0]
    res = np.asarray(out4, F).reshape(-1, K, 4)
    acc = np.zeros((res.shape[0], 4), F)
    with np.errstate(all="ignore"):
        for k in range(K):
            acc = fmaf(rows[k, 3], res[:, k], acc)
        acc[:, 3] = F(1.0) - acc[:, 3]
    return acc


def hostile_cones(n, g0, E):
    """Sixteen hand-written cones (tests/test_query.py item 3): legal inputs with a defined
    result.  Points are given in voxel units and converted to world units."""
    hh = F(E) / F(n)
    g = np.array(g0, F)
    w = lambda q: g + np.array(q, F) * hh                      # world point of voxel-unit q
    c = n / 2.0
    rows = [
        # p, d, tau, t_lim, off, valid
        (w((c, c, c)), (0.0, 0.0, -1.0), 0.3, INF, (0, 0, 0), 1.0),                    # plain, unit d
        (w((c, c, c)), (0.6, -1.7, 0.4), 0.02, INF, (0, 0, 0), 1.0),                   # non-unit d
        (w((c, c + 4.0, c + 2.0)), (0.0, 0.0, 0.0), 0.02, INF, (0, 0, 0), 1.0),        # zero d, in the open: t runs to t_max
        (w((c, 2.0, c)), (0.3, 0.2, -0.9), 1.0, INF, (1.5, 0.0, -2.0), 1.0),           # off not parallel to d
        (w((c, c, n - 2.0)), (0.1, -0.2, -1.0), 0.3, 0.5, (0, 0, 0), 1.0),             # t_lim 0.5: no step
        (w((c, c, n - 2.0)), (0.1, -0.2, -1.0), 0.3, 3.25, (0, 0, 0), 1.0),            # t_lim 3.25
        (w((c, c, n - 2.0)), (0.1, -0.2, -1.0), 0.3, NAN, (0, 0, 0), 1.0),             # NaN t_lim never limits
        (w((c, c, c)), (-1.0, 0.1, 0.2), NAN, INF, (0, 0, 0), 1.0),                    # NaN tau: TAU_MIN
        (w((c, c, c)), (-1.0, 0.1, 0.2), 0.0, INF, (0, 0, 0), 1.0),                    # tau 0: TAU_MIN
        (w((c, c, c)), (1.0, 0.1, -0.2), 7.0, INF, (0, 0, 0), 1.0),                    # tau 7: TAU_MAX
        ((NAN, 0.0, 0.0), (0.0, 1.0, 0.0), 0.3, INF, (0, 0, 0), 1.0),                  # NaN p
        ((INF, 0.0, -INF), (0.0, 1.0, 0.0), 0.3, INF, (0, 0, 0), 1.0),                 # infinite p
        (w((-3.0, c, c)), (1.0, 0.0, 0.0), 0.3, INF, (0, 0, 0), 1.0),                  # outside, aimed inside: no step
        (w((c, c, c)), (NAN, 1.0, 0.0), 0.3, INF, (0.0, INF, 0.0), 1.0),               # non-finite d and off
        (w((c, c, c)), (0.0, 0.0, -1.0), 0.3, INF, (0, 0, 0), 0.0),                    # valid 0
        (w((c, c, c)), (0.0, 0.0, -1.0), 0.3, INF, (0, 0, 0), -0.0),                   # valid -0
    ]
    return np.concatenate([make_cones(*r) for r in rows], axis=0)


# ---- the march ----------------------------------------------------------------------------------
def origins(n, g0, E, cones):
    """o_c = ((p_c - g0_c) * inv_h) + off_c for every cone."""
    cones = np.asarray(cones, F)
    inv_h = F(n) / F(E)
    with np.errstate(all="ignore"):
        o = (cones[:, 0:3] - np.array(g0, F)[None, :]) * inv_h + cones[:, 8:11]
    assert o.dtype == np.float32
    return o


def _sample(pyr, l, aniso, q, face, d2, n):
    """S_l(q), four channels, for the cones of one level: q [R, 3], face [R, 3], d2 [R, 3]."""
    nl = n >> l
    scale = F(2.0 ** -l)
    u = q * scale - F(0.5)
    fl = np.floor(u)
    i0 = fl.astype(np.int64)
    w1 = u - fl
    w = (F(1.0) - w1, w1)
    acc = np.zeros((q.shape[0], 4), F)
    faces = l != 0 and aniso
    vols = np.stack(pyr[l]) if faces else pyr[l][0]
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                x, y, z = i0[:, 0] + dx, i0[:, 1] + dy, i0[:, 2] + dz
                inside = (x >= 0) & (x < nl) & (y >= 0) & (y < nl) & (z >= 0) & (z < nl)
                xc, yc, zc = (np.clip(v, 0, nl - 1) for v in (x, y, z))
                wc = (w[dx][:, 0] * w[dy][:, 1]) * w[dz][:, 2]
                if faces:
                    tx, ty, tz = (vols[face[:, k], zc, yc, xc] for k in range(3))
                    v = fmaf(d2[:, 2:3], tz, fmaf(d2[:, 1:2], ty, d2[:, 0:1] * tx))
                else:
                    v = vols[zc, yc, xc]
                acc = np.where(inside[:, None], fmaf(wc[:, None], v, acc), acc).astype(F)   # outside: adds nothing
    return acc


def march(pyr, n, aniso, g0, E, cones):
    """vct_cone_query_device: -> dict(out4 [R, 4] float32, steps [R] int64, end [R] END_*, tau [R])."""
    cones = np.ascontiguousarray(cones, F).reshape(-1, 12)
    R = cones.shape[0]
    L = int(round(np.log2(n)))
    nf, Lf = F(n), F(L)
    tmax = F(n) * F(spec_ref.SQRT3)
    o = origins(n, g0, E, cones)
    d, t_lim = cones[:, 4:7], cones[:, 7]
    with np.errstate(all="ignore"):
        tau = np.fmin(np.fmax(cones[:, 3], TAU_MIN), TAU_MAX).astype(F)
        tau2 = F(2.0) * tau
        face = np.where(d >= 0, 0, 1) + np.array([0, 2, 4])[None, :]
        d2 = d * d
    out = np.zeros((R, 4), F)
    steps = np.zeros(R, np.int64)
    end = np.full(R, END_SKIPPED, np.int8)
    t = np.ones(R, F)
    act = np.flatnonzero(cones[:, 11] != 0)                    # a NaN valid is not 0
    end[act] = END_CAP
    with np.errstate(all="ignore"):
        for _ in range(MAX_STEPS):
            if not act.size:
                break
            # step 1, the tests in order
            stop = ~(out[act, 3] < ALPHA_STOP)
            end[act[stop]] = END_ALPHA
            act = act[~stop]
            far = ~(t[act] <= tmax)
            end[act[far]] = END_LEFT
            act = act[~far]
            lim = t[act] >= t_lim[act]
            end[act[lim]] = END_LIMIT
            act = act[~lim]
            q = o[act] + d[act] * t[act, None]
            inside = np.all((q >= 0) & (q <= nf), axis=1)
            end[act[~inside]] = END_LEFT
            act, q = act[inside], q[inside]
            if not act.size:
                break
            # step 2
            D = np.fmax(F(1.0), tau2[act] * t[act])
            m = np.fmin(log2(D), Lf)
            l0 = m.astype(np.int64)
            fr = m - l0.astype(F)
            # step 3
            s = np.zeros((act.size, 4), F)
            for l in np.unique(l0):
                k = np.flatnonzero(l0 == l)
                s[k] = _sample(pyr, int(l), aniso, q[k], face[act[k]], d2[act[k]], n)
            two = (fr > 0) & (l0 < L)
            for l in np.unique(l0[two]):
                k = np.flatnonzero(two & (l0 == l))
                s1 = _sample(pyr, int(l) + 1, aniso, q[k], face[act[k]], d2[act[k]], n)
                s[k] = fmaf(fr[k, None], s1, (F(1.0) - fr[k])[:, None] * s[k])
            # steps 4, 5
            oma = F(1.0) - out[act, 3]
            out[act] = fmaf(oma[:, None], s, out[act])
            t[act] = t[act] + F(spec_ref.STEP_SCALE) * D
            steps[act] += 1
    assert out.dtype == np.float32
    return {"out4": out, "steps": steps, "end": end, "tau": tau}


def coverage(res, cones):
    """Shares of the end classes over the valid cones, the most distinct apertures inside one
    group of 64 consecutive cones, and the longest march."""
    end = res["end"]
    valid = end != END_SKIPPED
    m = max(int(valid.sum()), 1)
    out = {"valid": int(valid.sum()), "longest": int(res["steps"].max(initial=0))}
    for code, name in END_NAMES.items():
        out[name] = float((end == code).sum()) / m
    bits = res["tau"].view(np.uint32)
    out["apertures"] = max((np.unique(bits[i:i + 64][valid[i:i + 64]]).size for i in range(0, end.size, 64)), default=0)
    return out


# ---- the probe grid -------------------------------------------------------------------------------
def check_grid(grid):
    """The input rule: True when the grid is legal."""
    o, s, dims = np.array(grid["origin"], F), F(grid["spacing"]), grid["dims"]
    return bool(np.isfinite(o).all() and np.isfinite(s) and s > 0 and all(1 <= int(v) <= PROBE_MAX_DIM for v in dims))


def probe_positions(grid):
    """P [dz, dy, dx, 3] = fmaf((float)i_c, spacing, origin_c)."""
    dx, dy, dz = (int(v) for v in grid["dims"])
    k, j, i = np.meshgrid(np.arange(dz), np.arange(dy), np.arange(dx), indexing="ij")
    idx = np.stack([i, j, k], axis=-1).astype(F)
    with np.errstate(all="ignore"):
        return fmaf(idx, F(grid["spacing"]), np.array(grid["origin"], F)[None, None, None, :])


AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], F)   # VCT_FACE_* order
AXES = AXES + F(0.0)                                                                   # the other components are +0


def probe_cones(grid):
    """The build's cone list: probe-major ([dz][dy][dx]), six faces each."""
    P = probe_positions(grid).reshape(-1, 3)
    return make_cones(np.repeat(P, 6, axis=0), np.tile(AXES, (P.shape[0], 1)), TAU_MAX, INF, 0.0, 1.0)


def probe_build(pyr, n, aniso, g0, E, albedo_occ, grid):
    """vct_probe_build_device: -> dict(probes [dz, dy, dx, 6, 4], state [dz, dy, dx] uint32, steps (int))."""
    dx, dy, dz = (int(v) for v in grid["dims"])
    cones = probe_cones(grid)
    res = march(pyr, n, aniso, g0, E, cones)
    o = origins(n, g0, E, cones[::6])
    occ = np.asarray(albedo_occ, F)[..., 3] != 0
    with np.errstate(all="ignore"):
        inside = np.all((o >= 0) & (o < F(n)), axis=1)
        v = np.where(inside[:, None], np.floor(o), 0).astype(np.int64)
    state = (inside & ~occ[v[:, 2], v[:, 1], v[:, 0]]).astype(np.uint32)
    return {"probes": res["out4"].reshape(dz, dy, dx, 6, 4), "state": state.reshape(dz, dy, dx),
            "steps": int(res["steps"].sum()), "cones": cones}


def probe_sample(grid, probes, state, pos4, nrm4):
    """vct_probe_sample_device: pos4, nrm4 [M, 4] -> (out4 [M, 4] float32, misses)."""
    pos4, nrm4 = (np.asarray(a, F).reshape(-1, 4) for a in (pos4, nrm4))
    probes, state = np.asarray(probes, F), np.asarray(state, np.uint32)
    dims = [int(v) for v in grid["dims"]]
    M = pos4.shape[0]
    origin, spacing = np.array(grid["origin"], F), F(grid["spacing"])
    valid = pos4[:, 3] != 0
    i0, w = [], []
    with np.errstate(all="ignore"):
        for c in range(3):
            g = (pos4[:, c] - origin[c]) / spacing
            g = np.fmin(np.fmax(g, F(0.0)), F(dims[c] - 1))
            lo = np.zeros(M, np.int64) if dims[c] == 1 else np.minimum(np.floor(g).astype(np.int64), dims[c] - 2)
            fr = g - lo.astype(F)
            i0.append(lo)
            w.append((F(1.0) - fr, fr))
        N = nrm4[:, :3]
        face = np.where(N >= 0, 0, 1) + np.array([0, 2, 4])[None, :]
        S = [np.zeros((M, 4), F) for _ in range(3)]
        W = np.zeros(M, F)
        rows = np.arange(M)
        for cn in range(8):
            dx, dy, dz = cn & 1, (cn >> 1) & 1, cn >> 2
            x, y, z = i0[0] + dx, i0[1] + dy, i0[2] + dz
            keep = (x < dims[0]) & (y < dims[1]) & (z < dims[2])
            xc, yc, zc = (np.minimum(v, dims[k] - 1) for k, v in enumerate((x, y, z)))
            keep &= state[zc, yc, xc] != 0
            wc = (w[0][dx] * w[1][dy]) * w[2][dz]
            W = np.where(keep, W + wc, W).astype(F)
            for a in range(3):
                pr = probes[zc, yc, xc, face[rows, a]]
                S[a] = np.where(keep[:, None], fmaf(wc[:, None], pr, S[a]), S[a]).astype(F)
        wn = N * N
        V = fmaf(wn[:, 2:3], S[2], fmaf(wn[:, 1:2], S[1], wn[:, 0:1] * S[0]))
        hit = W > 0
        out = np.zeros((M, 4), F)
        out[:, 3] = 1.0
        Ws = np.where(hit, W, F(1.0))
        q = V / Ws[:, None]
        out[hit, :3] = q[hit, :3]
        out[hit, 3] = (F(1.0) - q[:, 3])[hit]
        out[~valid] = 0.0
    assert out.dtype == np.float32
    return out, int((valid & ~hit).sum())


def grid_over(g0, E, d):
    """The grid ProbeGrid.over_aabb lays over a context's AABB: d probes per axis, the first and
    last half a spacing inside the box (one probe: at the centre)."""
    spacing = F(E) / F(d)
    origin = np.array(g0, F) + F(0.5) * spacing
    return {"origin": tuple(float(v) for v in origin), "spacing": float(spacing), "dims": (d, d, d)}
