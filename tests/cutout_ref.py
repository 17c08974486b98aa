"""Reference of the alpha cutouts (vct_spec.h "cutouts"; test infrastructure).

A numpy float32 restatement, one rounding per operation, of
  * the mask sample M_c(u, v): spec_ref.tex_sample's formula on channel c (`mask_scalar` is that
    function with a channel argument; `mask_sample` the same over arrays);
  * K1 with cutouts: spec_ref.voxelize's triangle loop with the coverage test in front of a
    pair's contribution (`voxelize`);
  * the frame: gbuffer_ref.nearest_hit restricted to accepted candidates (`nearest_hit`), and
    the records through gbuffer_ref.planes / shading_ref.planes for that (hit, t) (`frame`).
tests/test_cutout.py checks this file against the oracle on the cases where the mask cannot
matter, and by hand where it can.
"""
from __future__ import annotations

import math

import numpy as np

import gbuffer_ref as GR
import shading_ref as SHR
import spec_ref as SR

F = np.float32
fma = SHR.fmaf32


# ---------------------------------------------------------------------------
# the mask sample
# ---------------------------------------------------------------------------
def mask_scalar(t, u, v, c):
    """M_c(u, v) of an (H, W, 4) uint8 texture: spec_ref.tex_sample on channel c (scalar binary32)."""
    f32, lerp = SR.f32, SR._lerp
    H, W = t.shape[:2]
    u = float(u) if math.isfinite(u) else 0.0
    v = float(v) if math.isfinite(v) else 0.0
    fu, fv = f32(u - math.floor(u)), f32(v - math.floor(v))
    s, tt = f32(f32(fu * W) - 0.5), f32(f32(fv * H) - 0.5)
    sx, sy = math.floor(s), math.floor(tt)
    ax, ay = f32(s - sx), f32(tt - sy)
    x0, y0 = int(sx) % W, int(sy) % H
    x1, y1 = (int(sx) + 1) % W, (int(sy) + 1) % H
    px = lambda y, x: f32(float(t[y, x, c]) / 255.0)
    return lerp(lerp(px(y0, x0), px(y0, x1), ax), lerp(px(y1, x0), px(y1, x1), ax), ay)


def mask_sample(t, u, v, c):
    """The same over float32 arrays u, v -> float32 array."""
    t = np.asarray(t)
    H, W = t.shape[:2]
    u, v = np.asarray(u, F), np.asarray(v, F)
    with np.errstate(all="ignore"):
        u = np.where(np.isfinite(u), u, F(0))
        v = np.where(np.isfinite(v), v, F(0))
        fu, fv = u - np.floor(u), v - np.floor(v)
        s, tt = fu * F(W) - F(0.5), fv * F(H) - F(0.5)
        sx, sy = np.floor(s), np.floor(tt)
        ax, ay = s - sx, tt - sy
        x0, y0 = sx.astype(np.int64) % W, sy.astype(np.int64) % H
        x1, y1 = (sx.astype(np.int64) + 1) % W, (sy.astype(np.int64) + 1) % H
        px = lambda y, x: t[y, x, c].astype(F) / F(255)
        lerp = lambda a, b, f: fma(f, b - a, a)
        return lerp(lerp(px(y0, x0), px(y0, x1), ax), lerp(px(y1, x0), px(y1, x1), ax), ay).astype(F)


def covered(t, u, v, c, cutoff):
    """M_c(u, v) >= cutoff in float32."""
    return mask_sample(t, u, v, c) >= F(cutoff)


def interp_uv(uv6, b1, b2):
    """tri_uv over arrays: fmaf(b2, uv2 - uv0, fmaf(b1, uv1 - uv0, uv0)) per component; uv6 = u0 v0 u1 v1 u2 v2."""
    uv6 = np.asarray(uv6, F)
    with np.errstate(all="ignore"):
        return tuple(fma(b2, uv6[4 + k] - uv6[k], fma(b1, uv6[2 + k] - uv6[k], uv6[k])).astype(F) for k in range(2))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def voxel_bary(q, c):
    """spec_ref.tri_bary over arrays of voxel centres c = (cx, cy, cz); q: (3, 3) float32."""
    with np.errstate(all="ignore"):
        e1, e2 = [q[1, k] - q[0, k] for k in range(3)], [q[2, k] - q[0, k] for k in range(3)]
        w = [c[k] - q[0, k] for k in range(3)]
        d11, d12, d22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
        w1, w2 = _dot(w, e1), _dot(w, e2)
        den = d11 * d22 - d12 * d12
        z = np.zeros_like(c[0])
        if den > 0:
            b1, b2 = (d22 * w1 - d12 * w2) / den, (d11 * w2 - d12 * w1) / den
        else:
            b1, b2 = z, z
        b1, b2 = np.fmax(b1, F(0)), np.fmax(b2, F(0))
        s = b1 + b2
        over = s > 1
        return np.where(over, b1 / s, b1).astype(F), np.where(over, b2 / s, b2).astype(F)


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
def table_error(cutouts, n_tex, n_mat=None):
    """The table rule: None, or what is wrong.  cutouts: (map, channel, cutoff[, reserved]) per material."""
    if cutouts is None:
        return None
    if (len(cutouts) if n_mat is None else n_mat) == 0:
        return "n_materials == 0"
    for e in cutouts:
        m, ch, cut = e[:3]
        if m < -1 or m >= n_tex:
            return "map"
        if ch > 3:
            return "channel"
        if not (math.isfinite(cut) and 0 < F(cut) <= 1):
            return "cutoff"
        if len(e) > 3 and e[3] != 0:
            return "reserved"
    return None


def masks(cutouts, tri_mat, n_tri, has_uv=True):
    """Per triangle (map, channel, cutoff) or None (opaque)."""
    out = []
    for t in range(n_tri):
        e = None if cutouts is None or not has_uv else cutouts[0 if tri_mat is None else int(tri_mat[t])]
        out.append(None if e is None or e[0] < 0 else (int(e[0]), int(e[1]), F(e[2])))
    return out


# ---------------------------------------------------------------------------
# K1
# ---------------------------------------------------------------------------
def voxelize(n, g0, extent, verts, idx, tri_mat=None, kd4=None, mat_map=None, cutouts=None, textures=(), uv_offset=24):
    """spec_ref.voxelize with the coverage test -> (sums [n^3, 6] int64, counts [n^3] uint32,
    rejected = SAT-passing pairs that were not covered)."""
    g0 = np.asarray(g0, F)
    inv_h = F(n) / F(extent)
    sums = np.zeros((n ** 3, 6), np.int64)
    counts = np.zeros(n ** 3, np.int64)
    idx = np.asarray(idx).reshape(-1, 3)
    verts = np.asarray(verts, F)
    has_uv = uv_offset % 4 == 0 and uv_offset + 8 <= verts.shape[1] * 4
    mk = masks(cutouts, tri_mat, idx.shape[0], has_uv)
    rejected = 0
    for t, tri in enumerate(idx):
        m = 0 if tri_mat is None else int(tri_mat[t])
        kd = np.ones(3, F) if kd4 is None else np.asarray(kd4, F)[m, :3]
        p = verts[tri, :3]
        with np.errstate(all="ignore"):
            q = ((p - g0) * inv_h).astype(F)
        if not np.isfinite(q).all():            # a non-finite q: the triangle is skipped
            continue
        e1, e2 = p[1] - p[0], p[2] - p[0]
        fn = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]], F)
        ln = np.sqrt(SR._dot(*fn, *fn))
        fn = fn / ln if ln > 0 else np.zeros(3, F)
        fix = np.concatenate([SR._roundf(kd * F(65536)), SR._roundf(fn * F(65536))])
        lo, hi = [], []
        for a in range(3):
            mn, mx = np.fmin(np.fmin(q[0, a], q[1, a]), q[2, a]), np.fmax(np.fmax(q[0, a], q[1, a]), q[2, a])
            top = F(n) + F(1)
            lo.append(max(0, int(np.ceil(np.fmin(np.fmax(mn, F(-1)), top))) - 1))
            hi.append(min(n - 1, int(np.floor(np.fmax(np.fmin(mx, top), F(-1))))))
        if any(l > h for l, h in zip(lo, hi)):
            continue
        zz, yy, xx = np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in (2, 1, 0)], indexing="ij")
        c = [ar.astype(F) + F(0.5) for ar in (xx, yy, zz)]
        hit = SR._sat(q, *c)
        tex = -1 if mat_map is None else int(mat_map[m])
        if tex < 0 and mk[t] is None:
            v = (xx + n * (yy + n * zz))[hit]
            np.add.at(sums, v, fix[None, :])
            np.add.at(counts, v, 1)
            continue
        # the point of each pair: the voxel centre's projection, and its TexCoords
        uv6 = verts[tri, uv_offset // 4: uv_offset // 4 + 2].reshape(-1)
        ch = [a[hit] for a in c]
        b1, b2 = voxel_bary(q, ch)
        u, w = interp_uv(uv6, b1, b2)
        keep = np.ones(b1.shape, bool)
        if mk[t] is not None:
            keep = covered(textures[mk[t][0]], u, w, mk[t][1], mk[t][2])
            rejected += int((~keep).sum())
        v = (xx + n * (yy + n * zz))[hit][keep]
        add = np.tile(fix, (v.size, 1))
        if tex >= 0:   # albedo = Kd x T(uv), per covered pair
            for k in range(3):
                with np.errstate(all="ignore"):
                    add[:, k] = SR._roundf(((kd[k] * mask_sample(textures[tex], u[keep], w[keep], k)) * F(65536)).astype(F))
        np.add.at(sums, v, add)
        np.add.at(counts, v, 1)
    return sums, counts.astype(np.uint32), rejected


# ---------------------------------------------------------------------------
# the frame
# ---------------------------------------------------------------------------
def _accepted(rec_k, P, d, uv6, mask, textures, n_tex, cand):
    """Coverage of triangle k's candidate pixels (cand [h, w] bool) -> bool [h, w]."""
    if mask is None or mask[0] >= n_tex:        # opaque, or a stale mask index: no mask
        return cand
    with np.errstate(all="ignore"):
        _, _, b1, b2 = GR._mt(rec_k, P, d)
        u, v = interp_uv(uv6, b1, b2)
    return cand & covered(textures[mask[0]], u, v, mask[1], mask[2])


def nearest_hit(rec, cam, w, h, uv, mk, textures, n_tex=None, order=None):
    """gbuffer_ref.nearest_hit over the accepted candidates -> (hit, best, d, evals).  uv: [n, 6];
    mk: per triangle (map, channel, cutoff) or None; order: the triangles' visiting order (default
    ascending; any order gives the same frame: the winner is the smallest accepted t, ties to the
    lower index).  evals: mask evaluations when only would-be winners are tested."""
    n_tex = len(textures) if n_tex is None else n_tex
    d = GR.pixel_rays(cam, w, h)
    P = np.asarray(cam.position, F)
    best = np.full((h, w), np.inf, F)
    hit = np.full((h, w), -1, np.int32)
    evals = 0
    with np.errstate(all="ignore"):
        for k in (range(rec.shape[0]) if order is None else order):
            if not rec[k, 1:].any():
                continue
            miss, t, _, _ = GR._mt(rec[k], P, d)
            cand = ~miss & (t > 0) & ((t < best) | ((t == best) & (k < hit)))
            if mk[k] is not None and mk[k][0] < n_tex:
                evals += int(cand.sum())
            win = _accepted(rec[k], P, d, uv[k], mk[k], textures, n_tex, cand)
            best = np.where(win, t, best)
            hit = np.where(win, np.int32(k), hit)
    return hit, best, d, evals


class _Spec:
    """spec_ref's scalar binary32 tri_uv and tex_sample behind gbuffer_ref.planes' `oracle`
    argument (they take Python floats: numpy float32 scalars would round their exact products)."""
    tri_uv = staticmethod(lambda uv, b1, b2: SR.tri_uv([float(x) for x in uv], float(b1), float(b2)))
    tex_sample = staticmethod(lambda t, u, v: SR.tex_sample(t, float(u), float(v)))


def frame(rec, kd, cam, w, h, rough, uv, mk, textures, tex_of=None, n_tex=None, at=None):
    """The planes of vct_gbuffer_cutout_device: flat (at None: pos, nrm, alb) or shaded (at: a
    shading_ref.Attrs; the seven planes), and the winners."""
    n_tex = len(textures) if n_tex is None else n_tex
    hit, best, d, evals = nearest_hit(rec, cam, w, h, uv, mk, textures, n_tex)
    if tex_of is not None:                       # a stale diffuse map is no map (write_gbuffer)
        tex_of = np.where(np.asarray(tex_of) < n_tex, tex_of, -1)
    if at is None:
        pos, nrm, alb = GR.planes(rec, kd, cam, w, h, rough, hit, best, d, tex_of=tex_of, uv=uv, textures=textures, oracle=_Spec)
        out = {"pos": pos, "nrm": nrm, "alb": alb}
    else:
        out = SHR.planes(rec, kd, cam, w, h, rough, at, textures, n_tex=n_tex, hit=hit, best=best, d=d, tex_of=tex_of,
                         uv=uv, oracle=_Spec)
    out["hit"], out["evals"] = hit, evals
    return out


# ---------------------------------------------------------------------------
# the catalogue's references, computed once and left unchanged
# ---------------------------------------------------------------------------
_cache = {}


def _frozen(key, make):
    if key not in _cache:
        out = make()
        for a in (out.values() if isinstance(out, dict) else out):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def case_k1(case):
    """(sums, counts, rejected) of a cutout_inputs.Case (its static mesh)."""
    import cutout_inputs as CI

    def make():
        v, i, m, kd, mm, cuts = case.mesh.arrays(case.table)
        return voxelize(case.n, CI.G0, CI.E, v, i, m, kd, mm, cuts, case.textures)
    return _frozen(("k1", case.name), make)


def materials(case):
    """A shading material per triangle of the case: distinct Ks and roughness, no maps."""
    from vct.shading import ShadingMaterial
    return [ShadingMaterial(ks=(0.25 + t % 3, 0.5, 1.0 / (1 + t % 7)), roughness=0.05 + 0.1 * (t % 9)) for t in
            range(case.mesh.n_tri)]


def case_frame(case, shaded, solid=False):
    """frame() of a cutout_inputs.Case: flat or shaded records; solid: with every mask ignored
    (what the existing passes write)."""
    import cutout_inputs as CI

    def make():
        v, i, m, kd4, mm, cuts = case.mesh.arrays(case.table and not solid)
        n_static = i.size // 3
        mk = masks(cuts, m, n_static)
        kd = kd4[m][:, :3]
        tex_of = np.full(n_static, -1, np.int64) if mm is None else np.asarray(mm, np.int64)[m]
        at = SHR.Attrs.from_verts(v, i, materials(case), m) if shaded else None
        if case.dynamic is not None:
            dv, di = case.dynamic.arrays()[:2]
            i = np.concatenate([i, di + np.uint32(v.shape[0])])
            v = np.concatenate([v, dv])
            nd = di.size // 3
            kd = np.concatenate([kd, np.broadcast_to(CI.DYN_KD[:3], (nd, 3))])
            mk += [None] * nd
            tex_of = np.concatenate([tex_of, np.full(nd, -1, np.int64)])
        rec = GR.k1_skip(GR.tri_records(v, i), v, i, case.n, CI.G0, CI.E)
        uv = np.asarray(v, F)[np.asarray(i, np.int64).reshape(-1, 3)][..., 6:8].reshape(-1, 6)
        return frame(rec, kd.astype(F), case.cam, case.w, case.h, CI.ROUGH, uv, mk, case.textures,
                     tex_of=tex_of if (tex_of >= 0).any() else None, n_tex=case.n_tex_after, at=at)
    return _frozen(("frame", case.name, shaded, solid), make)
