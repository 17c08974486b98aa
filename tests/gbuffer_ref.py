"""References of the two G-buffer passes (vct_spec.h "G-buffer input rule"; test infrastructure).

Two parts:

* a numpy float32 restatement, one rounding per operation, of pixel_ray, ray_tri, the
  nearest-hit loop and write_gbuffer (csrc/vct_frame.hip, csrc/vct_view.h) -> the winning
  triangle and t per pixel and the three planes, and of k_bin_rect -> the tile rectangle per
  triangle.  `bin_rects(..., parent=True)` restates k_bin_rect as it was before the rule was
  written (far cull on the vertices' cz, no whole-frame rectangle, a fixed margin), which
  tests/test_gbuffer_inputs.py uses to show the two findings;
* a float64 caster with a per-pixel robustness margin, for the comparison that does not
  depend on float32 rounding.

tan_half is libm's tanf (both backends call it on the host; numpy's float32 tan is another
implementation).
"""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

F = np.float32
ZC = F(1e-5)
TILE = 16
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.restype = ctypes.c_float
_libm.tanf.argtypes = [ctypes.c_float]


def tan_half(zoom_deg) -> np.float32:
    """tanf(zoom_deg * 0.5f * 3.14159265358979f / 180.0f)"""
    with np.errstate(all="ignore"):
        return F(_libm.tanf(F(zoom_deg) * F(0.5) * F(3.14159265358979) / F(180.0)))


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def tri_records(verts, idx):
    """[n, 3, 3] float32: v0, e1 = v1 - v0, e2 = v2 - v0 (k1_tri_setup), before the K1 skip."""
    p = np.asarray(verts, F)[:, :3][np.asarray(idx).reshape(-1, 3)]
    with np.errstate(all="ignore"):
        return np.stack([p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]], 1).astype(F)


def k1_skip(rec, verts, idx, n, g0, extent):
    """The K1 input rule: a triangle with a non-finite q = (p - g0) * (n / E) is an all-zero record."""
    p = np.asarray(verts, F)[:, :3][np.asarray(idx).reshape(-1, 3)]
    with np.errstate(all="ignore"):
        q = (p - np.asarray(g0, F)) * (F(n) / F(extent))
    rec = rec.copy()
    rec[~np.isfinite(q).all((1, 2))] = 0
    return rec


def pixel_rays(cam, w, h):
    """[h, w, 3] float32 unit ray directions (vct_view.h pixel_ray)."""
    th, aspect = tan_half(cam.zoom), F(w) / F(h)
    x = np.arange(w, dtype=F)[None, :]
    y = np.arange(h, dtype=F)[:, None]
    ndx = (F(2) * (x + F(0.5)) / F(w) - F(1)) * th * aspect
    ndy = (F(1) - F(2) * (y + F(0.5)) / F(h)) * th
    f, u, r = (np.asarray(v, F) for v in (cam.front, cam.up, cam.right))
    d = [(f[k] + ndx * r[k]) + ndy * u[k] for k in range(3)]
    il = F(1) / np.sqrt(dot3(d[0], d[1], d[2], d[0], d[1], d[2]))
    return np.stack([d[0] * il, d[1] * il, d[2] * il], -1).astype(F)


def _mt(rec, P, d):
    """Moller-Trumbore terms of one triangle over all pixels -> (miss, t, u, v), float32."""
    v0, e1, e2 = rec
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    pvx, pvy, pvz = dy * e2[2] - dz * e2[1], dz * e2[0] - dx * e2[2], dx * e2[1] - dy * e2[0]
    det = dot3(e1[0], e1[1], e1[2], pvx, pvy, pvz)
    inv = F(1) / det
    tx, ty, tz = P[0] - v0[0], P[1] - v0[1], P[2] - v0[2]
    u = dot3(tx, ty, tz, pvx, pvy, pvz) * inv
    qx, qy, qz = ty * e1[2] - tz * e1[1], tz * e1[0] - tx * e1[2], tx * e1[1] - ty * e1[0]
    v = dot3(dx, dy, dz, qx, qy, qz) * inv
    t = dot3(e2[0], e2[1], e2[2], qx, qy, qz) * inv
    miss = (np.abs(det) < F(1e-12)) | (u < 0) | (u > 1) | (v < 0) | (u + v > 1)
    return miss, t, u, v


def nearest_hit(rec, cam, w, h):
    """The caster's loop: -> (hit [h, w] int32, -1 = none; best [h, w] float32; d [h, w, 3])."""
    d = pixel_rays(cam, w, h)
    P = np.asarray(cam.position, F)
    best = np.full((h, w), np.inf, F)
    hit = np.full((h, w), -1, np.int32)
    with np.errstate(all="ignore"):
        for k in range(rec.shape[0]):
            if not rec[k, 1:].any():
                continue                     # an all-zero edge pair: det == 0, never a hit
            miss, t, _, _ = _mt(rec[k], P, d)
            win = ~miss & (t > 0) & (t < best)
            best = np.where(win, t, best)
            hit = np.where(win, np.int32(k), hit)
    return hit, best, d


def planes(rec, kd, cam, w, h, rough, hit, best, d, tex_of=None, uv=None, textures=None, oracle=None):
    """write_gbuffer over the frame -> (pos4, nrm4, alb4) float32 [h, w, 4].
    kd: [n, 3] per triangle; tex_of: [n] texture index or -1; uv: [n, 6]."""
    P, Fr = np.asarray(cam.position, F), np.asarray(cam.front, F)
    with np.errstate(all="ignore"):
        depth = best * dot3(d[..., 0], d[..., 1], d[..., 2], Fr[0], Fr[1], Fr[2])
        bg = (hit < 0) | (depth < F(cam.near)) | (depth > F(cam.far))
        k = np.where(hit < 0, 0, hit)
        e1, e2 = rec[k, 1], rec[k, 2]
        nx = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
        ny = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
        nz = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
        nl = np.sqrt(dot3(nx, ny, nz, nx, ny, nz))
        nx, ny, nz = nx / nl, ny / nl, nz / nl
        flip = dot3(nx, ny, nz, d[..., 0], d[..., 1], d[..., 2]) > 0
        nx, ny, nz = (np.where(flip, -a, a) for a in (nx, ny, nz))
        pos = np.stack([P[0] + d[..., 0] * best, P[1] + d[..., 1] * best, P[2] + d[..., 2] * best,
                        np.ones((h, w), F)], -1)
        nrm = np.stack([nx, ny, nz, np.zeros((h, w), F)], -1)
        alb = np.concatenate([np.asarray(kd, F)[k], np.full((h, w, 1), F(rough))], -1)
        if tex_of is not None:
            for y, x in np.argwhere(~bg & (np.asarray(tex_of)[k] >= 0)):
                t = int(hit[y, x])
                _, _, b1, b2 = _mt(rec[t], P, d[y, x])
                u, v = oracle.tri_uv(uv[t], b1, b2)
                alb[y, x, :3] = np.asarray(kd, F)[t] * np.asarray(oracle.tex_sample(textures[tex_of[t]], u, v), F)
    pos, nrm, alb = (a.astype(F) for a in (pos, nrm, alb))
    pos[bg] = 0
    nrm[bg] = 0
    alb[bg, :3] = 0
    return pos, nrm, alb


def bin_rects(rec, cam, w, h, parent=False, boxes=False):
    """k_bin_rect: [n, 4] int32 tile rectangles (x0, y0, x1, y1), x0 > x1 = culled.
    boxes: also the projected boxes before the margin, float32 [n, 4] (lo_x, lo_y, hi_x, hi_y),
    and which triangles got the whole frame."""
    th, aspect = tan_half(cam.zoom), F(w) / F(h)
    tiles_x, tiles_y = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    with np.errstate(all="ignore"):
        sxs = F(0.5) * F(w) / (th * aspect)
        sys_ = F(0.5) * F(h) / th
        ext = th * aspect
        t_near = F(2) * ZC * np.sqrt(F(1) + ext * ext + th * th)
        reach = F(1) + th + ext
        pad = F(9.5367431640625e-07) * sys_ * reach * reach
        P, f, u, r = (np.asarray(v, F) for v in (cam.position, cam.front, cam.up, cam.right))
        v0, e1, e2 = rec[:, 0], rec[:, 1], rec[:, 2]
        n = rec.shape[0]
        c = np.zeros((3, n, 3), F)
        for i, v in enumerate((v0, v0 + e1, v0 + e2)):
            q = v - P
            for j, ax in enumerate((r, u, f)):
                c[i, :, j] = dot3(q[:, 0], q[:, 1], q[:, 2], ax[0], ax[1], ax[2])
        lo = np.full((2, n), np.inf, F)
        hi = np.full((2, n), -np.inf, F)
        anyp = np.zeros(n, bool)
        below = np.zeros(n, bool)
        beyond = np.ones(n, bool)

        def put(p0, p1, p2, sel):
            X = F(0.5) * F(w) + (p0 / p2) * sxs
            Y = F(0.5) * F(h) - (p1 / p2) * sys_
            for a, val in ((0, X), (1, Y)):
                lo[a] = np.where(sel, np.fmin(lo[a], val), lo[a])
                hi[a] = np.where(sel, np.fmax(hi[a], val), hi[a])
            anyp[:] |= sel

        for i in range(3):
            a, b = c[i], c[(i + 1) % 3]
            beyond &= a[:, 2] > F(cam.far)
            ina, inb = a[:, 2] >= ZC, b[:, 2] >= ZC
            below |= ~ina
            put(a[:, 0], a[:, 1], a[:, 2], ina)
            s = (ZC - a[:, 2]) / (b[:, 2] - a[:, 2])
            put(a[:, 0] + (b[:, 0] - a[:, 0]) * s, a[:, 1] + (b[:, 1] - a[:, 1]) * s, np.full(n, ZC, F), ina != inb)
        full = np.zeros(n, bool)
        grow = np.zeros(n, F)
        edges = np.ones(n, bool)
        if parent:
            anyp &= ~beyond
        else:
            edges = (e1 != 0).any(1) & (e2 != 0).any(1)
            l1 = np.sqrt(dot3(e1[:, 0], e1[:, 1], e1[:, 2], e1[:, 0], e1[:, 1], e1[:, 2]))
            l2 = np.sqrt(dot3(e2[:, 0], e2[:, 1], e2[:, 2], e2[:, 0], e2[:, 1], e2[:, 2]))
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            t = v0 - P
            dn = np.abs(dot3(t[:, 0], t[:, 1], t[:, 2], nx, ny, nz))
            nl = np.sqrt(dot3(nx, ny, nz, nx, ny, nz))
            lt = np.sqrt(dot3(t[:, 0], t[:, 1], t[:, 2], t[:, 0], t[:, 1], t[:, 2]))
            grow = pad * (np.fmax(lt, np.fmax(l1, l2)) * (l1 * l2) / dn)
            full = ~(grow < F(32768))
            clear = (nl > F(1e-30)) & (dn > t_near * nl + F(9.5367431640625e-07) * (lt + t_near) * (l1 * l2))
            full |= below & ~clear
            full &= edges
        x0, x1 = np.fmax(lo[0] - F(1.5) - grow, F(0)), np.fmin(hi[0] + F(0.5) + grow, F(w - 1))
        y0, y1 = np.fmax(lo[1] - F(1.5) - grow, F(0)), np.fmin(hi[1] + F(0.5) + grow, F(h - 1))
        ok = anyp & (x0 <= x1) & (y0 <= y1) & ~full & edges
        rc = np.tile(np.array([1, 0, 0, 0], np.int32), (n, 1))
        z = lambda a: np.where(ok, a, 0).astype(np.int32) // TILE
        rc[ok] = np.stack([z(x0), z(y0), z(x1), z(y1)], 1)[ok]
        rc[full] = (0, 0, tiles_x - 1, tiles_y - 1)
    return (rc, np.stack([lo[0], lo[1], hi[0], hi[1]], 1), full) if boxes else rc


def margin_used(hit, box, full):
    """How far outside its winner's projected box each pixel centre lies, in pixels (0 inside; the
    kernel allows one pixel) -> float64 [h, w]; pixels without a winner or whose winner has the
    whole frame count 0."""
    h, w = hit.shape
    y, x = np.mgrid[0:h, 0:w] + 0.5
    b = box[np.where(hit < 0, 0, hit)].astype(np.float64)
    out = np.maximum.reduce([b[..., 0] - x, x - b[..., 2], b[..., 1] - y, y - b[..., 3], np.zeros((h, w))])
    return np.where((hit < 0) | full[np.where(hit < 0, 0, hit)], 0.0, out)


def outside_rect(hit, rc):
    """Pixels whose winning triangle's rectangle does not hold their tile -> bool [h, w]."""
    h, w = hit.shape
    ty, tx = np.mgrid[0:h, 0:w] // TILE
    r = rc[np.where(hit < 0, 0, hit)]
    inside = (r[..., 0] <= tx) & (tx <= r[..., 2]) & (r[..., 1] <= ty) & (ty <= r[..., 3])
    return (hit >= 0) & ~inside


# ---------------------------------------------------------------------------
# float64 caster with a robustness margin
# ---------------------------------------------------------------------------
def cast64(rec, cam, w, h):
    """The same definition in float64 (ideal pixel-centre rays, the float32 inputs taken exactly).
    -> dict(hit, valid, t, d) and the per-pixel robustness terms:
       edge   min(u, v, 1 - u - v) of the nearest hit: its distance from the triangle's edges in
              barycentrics (a triangle of zero area is never hit and has no say);
       miss   over the triangles not hit (with t > 0): how far outside the nearest miss was, in the
              same units; 0 where a triangle's answer is undefined (the ray lies in its plane);
       gap_t  relative gap of the nearest t to the second nearest;
       gap_z  relative gap of the depth to near_plane and to far_plane;
       ndet   |det| / (|e1| |e2|) of the nearest hit.
    `robust(r, thr)` is the pixels where all of them clear their thresholds."""
    D = np.float64
    rec = np.asarray(rec, D)
    f, u_, r = (np.asarray(v, F).astype(D) for v in (cam.front, cam.up, cam.right))
    P = np.asarray(cam.position, F).astype(D)
    th = np.tan(D(F(cam.zoom)) * 0.5 * np.pi / 180.0)
    x = np.arange(w, dtype=D)[None, :]
    y = np.arange(h, dtype=D)[:, None]
    ndx = (2 * (x + 0.5) / w - 1) * th * (w / h)
    ndy = (1 - 2 * (y + 0.5) / h) * th
    d = np.stack([f[k] + ndx * r[k] + ndy * u_[k] for k in range(3)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    best = np.full((h, w), np.inf)
    second = np.full((h, w), np.inf)
    hit = np.full((h, w), -1, np.int32)
    edge = np.full((h, w), np.inf)
    miss = np.full((h, w), np.inf)
    ndet = np.full((h, w), np.inf)
    with np.errstate(all="ignore"):
        for k in range(rec.shape[0]):
            v0, e1, e2 = rec[k]
            if not np.isfinite(rec[k]).all() or not np.cross(e1, e2).any():
                continue                     # K1 skips it / zero area: no ray hits it
            scale = np.linalg.norm(e1) * np.linalg.norm(e2)
            pv = np.cross(d, e2)
            det = pv @ e1
            T = P - v0
            q = np.cross(T, e1)
            nu, nv, nt = pv @ T, d @ q, q @ e2
            uu, vv, t = nu / det, nv / det, nt / det
            bary = np.minimum(np.minimum(uu, vv), 1 - uu - vv)
            par = det == 0                   # the ray is parallel to the plane: a miss, unless it lies in it
            in_plane = par & (np.maximum(np.abs(nu), np.abs(nv)) <= 1e-9 * scale * np.linalg.norm(T))
            inside = ~par & (bary >= 0) & (t > 0)
            out = ~par & ~inside & (t > 0)
            miss = np.where(out, np.minimum(miss, -bary), miss)
            miss = np.where(in_plane | (~par & ~np.isfinite(bary)), 0.0, miss)
            newbest = inside & (t < best)
            second = np.where(newbest, best, np.where(inside, np.minimum(second, t), second))
            edge = np.where(newbest, bary, edge)
            ndet = np.where(newbest, np.abs(det) / scale, ndet)
            hit = np.where(newbest, np.int32(k), hit)
            best = np.where(newbest, t, best)
        depth = best * (d @ f)
        near, far = D(F(cam.near)), D(F(cam.far))
        valid = (hit >= 0) & (depth >= near) & (depth <= far)
        none = hit < 0
        gap_t = np.where(np.isfinite(second), (second - best) / second, np.inf)
        gap_z = np.where(none, np.inf, np.minimum(np.abs(depth - near), np.abs(depth - far)) / np.abs(depth))
    return {"hit": hit, "valid": valid, "t": best, "d": d, "edge": np.where(none, np.inf, edge), "miss": miss,
            "gap_t": gap_t, "gap_z": gap_z, "ndet": np.where(none, np.inf, ndet)}


# thresholds of the terms that do not depend on the case: float32 evaluates t and the depth to a
# few 2^-24 relative (x 1 / ndet), so a relative gap of 2^-16 and a normalised determinant of
# 2^-10 leave a factor of 2^5 and more
GAP_T = GAP_Z = 2.0 ** -16
NDET = 2.0 ** -10


def robust(r, thr):
    """Pixels whose float64 answer float32 rounding cannot change: thr is the case's margin in
    barycentric units (the rounding of u and v grows with |eye - v0| / |edge|)."""
    return (r["edge"] > thr) & (r["miss"] > thr) & (r["gap_t"] > GAP_T) & (r["gap_z"] > GAP_Z) & (r["ndet"] > NDET)
