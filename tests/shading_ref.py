"""Reference of the shading G-buffer (vct_spec.h "shading attributes"; test infrastructure).

A numpy restatement of the per-pixel rule of vct_gbuffer_shaded_device, one rounding per
operation, built on gbuffer_ref (the hit, pos4, the face normal and the albedo are
gbuffer_ref.nearest_hit / planes themselves) and on spec_ref.tex_sample.  The rule is written
once, over a number format: `planes` runs it in float32 (fmaf = one rounding), `planes64` runs
the same formulas in float64 on gbuffer_ref.cast64's hits, for the comparison that does not
depend on float32 rounding.
"""
from __future__ import annotations

import math

import numpy as np

import gbuffer_ref as GR
import spec_ref as SR

F = np.float32
NO_HIT = 0xFFFFFFFF


def fmaf32(a, b, c):
    """Correctly rounded binary32 fma over arrays (spec_ref.fmaf's method: the product is exact in
    binary64, TwoSum makes the sum exact, the binary32 rounding is corrected at ties)."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        r = s.astype(F)
        r64 = r.astype(np.float64)
        below = r64 < s
        up, down = np.nextafter(r, F(np.inf)).astype(np.float64), np.nextafter(r, F(-np.inf)).astype(np.float64)
        lo, hi = np.where(below, r64, down), np.where(below, up, r64)
        tie = np.isfinite(s) & (err != 0) & (r64 != s) & (s - lo == hi - s)
        fixed = np.where(err > 0, hi, lo).astype(F)
    return np.where(tie, fixed, r)


def _tex64(t, u, v):
    """spec_ref.tex_sample's formulas in float64."""
    H, W = t.shape[:2]
    u = float(u) if math.isfinite(u) else 0.0
    v = float(v) if math.isfinite(v) else 0.0
    fu, fv = u - math.floor(u), v - math.floor(v)
    s, tt = fu * W - 0.5, fv * H - 0.5
    sx, sy = math.floor(s), math.floor(tt)
    ax, ay = s - sx, tt - sy
    x0, y0, x1, y1 = int(sx) % W, int(sy) % H, (int(sx) + 1) % W, (int(sy) + 1) % H
    px = lambda y, x, c: float(t[y, x, c]) / 255.0
    lerp = lambda a, b, f: a + f * (b - a)
    return [lerp(lerp(px(y0, x0, c), px(y0, x1, c), ax), lerp(px(y1, x0, c), px(y1, x1, c), ax), ay) for c in range(3)]


class Attrs:
    """The shading set: per-triangle vertex attributes ([n_set, 3, 3]; uv [n_set, 3, 2]; None =
    absent), a material per triangle and the material table (records with ks, roughness,
    normal_map, specular_map, flip_green: vct.shading.ShadingMaterial)."""

    def __init__(self, n_set, materials, tri_material=None, normal=None, uv=None, tangent=None, bitangent=None):
        self.n_set, self.materials = int(n_set), list(materials)
        self.tri_material = np.zeros(n_set, np.int64) if tri_material is None else np.asarray(tri_material, np.int64)
        self.normal, self.uv, self.tangent, self.bitangent = (
            None if a is None else np.asarray(a, F) for a in (normal, uv, tangent, bitangent))

    @staticmethod
    def from_verts(verts, idx, materials, tri_material=None, normal=True, uv=True, tangent=True, bitangent=True):
        """From the 14-float Vertex rows that vct_set_shading reads at offsets 12 / 24 / 32 / 44."""
        v = np.asarray(verts, F)[np.asarray(idx, np.int64).reshape(-1, 3)]
        return Attrs(v.shape[0], materials, tri_material, v[..., 3:6] if normal else None, v[..., 6:8] if uv else None,
                     v[..., 8:11] if tangent else None, v[..., 11:14] if bitangent else None)


def _interp(T, fma, a, k, b1, b2):
    """fmaf(b2, a2 - a0, fmaf(b1, a1 - a0, a0)) per component; a: [n, 3 vertices, c]."""
    a = a.astype(T)[k]
    with np.errstate(all="ignore"):
        return fma(b2[..., None], a[..., 2, :] - a[..., 0, :], fma(b1[..., None], a[..., 1, :] - a[..., 0, :], a[..., 0, :]))


def _unit(v):
    """v / sqrt(dot3(v, v)) and where the square is finite and > 0."""
    with np.errstate(all="ignore"):
        sq = GR.dot3(v[..., 0], v[..., 1], v[..., 2], v[..., 0], v[..., 1], v[..., 2])
        return v / np.sqrt(sq)[..., None], np.isfinite(sq) & (sq > 0)


def _shade(T, fma, tex, hit, lit, d, ng, flipped, b1, b2, at, textures, n_tex, rough):
    """Steps 3-7 of the rule over the frame in number format T -> (N [h, w, 3], ks [h, w, 3],
    alb_w [h, w], N1 [h, w, 3]).  lit: the pixels with a hit (not background); ng: the face normal
    as written (flipped toward the viewer); flipped: where it was negated."""
    h, w = hit.shape
    n_tex = len(textures) if n_tex is None else n_tex
    inset = lit & (hit < at.n_set)
    k = np.where(inset, hit, 0)
    sign = np.where(flipped, T(-1), T(1))[..., None]
    n0 = ng                                                   # step 3
    if at.normal is not None and at.n_set:
        u, ok = _unit(_interp(T, fma, at.normal, k, b1, b2))
        n0 = np.where(ok[..., None], u * sign, ng)
    n1 = n0.copy()
    ks = np.ones((h, w, 3), T)
    alb_w = np.full((h, w), T(rough), T)
    uv = _interp(T, fma, at.uv, k, b1, b2) if (at.uv is not None and at.n_set) else None
    frame = at.tangent is not None and at.bitangent is not None and at.n_set
    if frame:
        tg, bt = _interp(T, fma, at.tangent, k, b1, b2) * sign, _interp(T, fma, at.bitangent, k, b1, b2) * sign
    for y, x in np.argwhere(inset):
        m = at.materials[at.tri_material[k[y, x]]]
        alb_w[y, x] = T(F(m.roughness))
        ks[y, x] = np.asarray(m.ks, F).astype(T)
        if uv is not None and 0 <= m.specular_map < n_tex:
            ks[y, x] = ks[y, x] * np.asarray(tex(textures[m.specular_map], uv[y, x, 0], uv[y, x, 1]), T)
        if uv is not None and frame and 0 <= m.normal_map < n_tex:    # step 4
            c = np.asarray(tex(textures[m.normal_map], uv[y, x, 0], uv[y, x, 1]), T)
            mm = np.asarray(fma(T(2), c, T(-1)), T)
            if m.flip_green:
                mm[1] = -mm[1]
            with np.errstate(all="ignore"):
                v = (mm[0] * tg[y, x] + mm[1] * bt[y, x]) + mm[2] * n0[y, x]
            u, ok = _unit(v)
            if ok:
                n1[y, x] = u
    with np.errstate(all="ignore"):                           # step 5
        toward = GR.dot3(n1[..., 0], n1[..., 1], n1[..., 2], d[..., 0], d[..., 1], d[..., 2]) < 0
    return np.where((toward & inset)[..., None], n1, ng), np.where(inset[..., None], ks, T(1)), alb_w, n1


def _face(rec, k, d):
    """write_gbuffer's face normal before the flip, and whether it is flipped."""
    with np.errstate(all="ignore"):
        e1, e2 = rec[k, 1], rec[k, 2]
        nx = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
        ny = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
        nz = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
        nl = np.sqrt(GR.dot3(nx, ny, nz, nx, ny, nz))
        n = np.stack([nx / nl, ny / nl, nz / nl], -1)
        return n, GR.dot3(n[..., 0], n[..., 1], n[..., 2], d[..., 0], d[..., 1], d[..., 2]) > 0


def planes(rec, kd, cam, w, h, rough, at, textures=(), n_tex=None, hit=None, best=None, d=None, tex_of=None, uv=None,
           oracle=None):
    """The seven planes of vct_gbuffer_shaded_device in float32 -> dict(pos, nrm, alb, ks, geo
    [h, w, 4] float32; tri_id [h, w] uint32; bary [h, w, 2] float32).  rec, kd, tex_of, uv, oracle:
    gbuffer_ref.planes' arguments (all triangles, the dynamic layer's included); textures: the
    vct_set_textures list; n_tex: the current texture count when a smaller set made indices stale."""
    if hit is None:
        hit, best, d = GR.nearest_hit(rec, cam, w, h)
    pos, geo, alb = GR.planes(rec, kd, cam, w, h, rough, hit, best, d, tex_of=tex_of, uv=uv, textures=textures, oracle=oracle)
    lit = pos[..., 3] != 0
    k = np.where(hit < 0, 0, hit)
    _, flipped = _face(rec, k, d)
    with np.errstate(all="ignore"):
        _, _, b1, b2 = GR._mt([np.moveaxis(rec[k, j], -1, 0) for j in range(3)], np.asarray(cam.position, F), d)
    N, ks, alb_w, _ = _shade(F, fmaf32, lambda t, u, v: SR.tex_sample(t, float(u), float(v)), hit, lit, d, geo[..., :3],
                             flipped, b1, b2, at, textures, n_tex, rough)
    z = np.zeros((h, w, 1), F)
    nrm = np.concatenate([N, z], -1).astype(F)
    ks4 = np.concatenate([ks, z + F(1)], -1).astype(F)
    alb = alb.copy()
    alb[..., 3] = np.where(lit, alb_w, F(rough))
    nrm[~lit] = 0
    ks4[~lit] = 0
    bary = np.stack([b1, b2], -1).astype(F)
    bary[~lit] = 0
    tri_id = np.where(lit, hit, -1).astype(np.int64).astype(np.uint32)
    return {"pos": pos, "nrm": nrm, "alb": alb, "ks": ks4, "geo": geo, "tri_id": tri_id, "bary": bary}


def planes64(rec, cam, w, h, rough, at, textures=(), n_tex=None):
    """The same formulas in float64 on gbuffer_ref.cast64's hits (the float32 inputs taken exactly)
    -> dict(N, ks [h, w, 3], alb_w, hit, valid, r = cast64's record for gbuffer_ref.robust)."""
    D = np.float64
    r = GR.cast64(rec, cam, w, h)
    hit, lit, d = r["hit"], r["valid"], r["d"]
    k = np.where(hit < 0, 0, hit)
    rec64 = np.asarray(rec, D)
    n, flipped = _face(rec64, k, d)
    ng = np.where(flipped[..., None], -n, n)
    with np.errstate(all="ignore"):
        _, _, b1, b2 = GR._mt([np.moveaxis(rec64[k, j], -1, 0) for j in range(3)],
                              np.asarray(cam.position, F).astype(D), d)
    N, ks, alb_w, _ = _shade(D, lambda a, b, c: a * b + c, _tex64, hit, lit, d, ng, flipped, b1, b2, at, textures, n_tex,
                             rough)
    return {"N": N, "ks": ks, "alb_w": alb_w, "hit": hit, "valid": lit, "r": r, "ng": ng}


def case_arrays(case):
    """(rec, kd per triangle, Attrs) of a shading_inputs.Case: the mesh records of the static
    triangles and, behind them, of its dynamic layer; the K1 skip applied."""
    import shading_inputs as SI
    verts, idx = case.verts, case.idx
    kd = case.kd4[case.tri_mat][:, :3]
    if case.dynamic is not None:
        dv, di = case.dynamic
        idx = np.concatenate([idx, di + np.uint32(verts.shape[0])])
        verts = np.concatenate([verts, dv])
        kd = np.concatenate([kd, np.broadcast_to(DYN_KD[:3], (di.size // 3, 3))])
    rec = GR.k1_skip(GR.tri_records(verts, idx), verts, idx, SI.N, SI.G0, SI.E)
    at = Attrs.from_verts(case.verts, case.idx, case.materials, case.tri_mat, **case.present)
    return rec, kd.astype(F), at


DYN_KD = np.array([0.125, 0.875, 0.375, 1.0], F)      # the Kd of a case's dynamic layer
_cache = {}


def case_planes(case):
    """planes() of a shading_inputs.Case, computed once and left unchanged."""
    import shading_inputs as SI
    if case.name not in _cache:
        rec, kd, at = case_arrays(case)
        out = planes(rec, kd, case.cam, case.w, case.h, SI.ROUGH, at, case.textures, n_tex=case.n_tex_after)
        for a in out.values():
            a.setflags(write=False)
        _cache[case.name] = out
    return _cache[case.name]
