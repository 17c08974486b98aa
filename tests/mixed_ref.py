"""numpy restatement of include/vct_spec.h "mixed-resolution trace" (include/vct_mixed.h):
pick, upsample (plane, hole list, stats), scatter, and the frame call built from a
full-resolution trace.  Every float operation is a float32 numpy scalar operation in the
spec's order, so the GPU kernels are compared with it bit for bit.
"""
import numpy as np

F = np.float32
NO_SOURCE = 0xFFFFFFFF
HOLE_W = 64
NORMAL_COS = F(0.9)


def low_size(w, h, f):
    return (w + f - 1) // f, (h + f - 1) // f


def max_holes_of(w, h, max_holes=0):
    return max_holes if max_holes else (w * h + 7) // 8


def tap_weights(x, f):
    """-> (X0, (weight of tap X0, weight of tap X0 + 1)) for full-resolution coordinate x."""
    t = 2 * x + 1 - f
    X0 = t // (2 * f)                      # floor division: -1 for t < 0
    r = t - 2 * f * X0
    return X0, (2 * f - r, r)


def pick(pos, nrm, alb, eye, f):
    """-> lo_pos, lo_nrm, lo_alb [hl][wl][4] float32 and lo_src [hl][wl] uint32."""
    pos, nrm, alb = (np.ascontiguousarray(a, F) for a in (pos, nrm, alb))
    h, w = pos.shape[:2]
    wl, hl = low_size(w, h, f)
    lo = [np.zeros((hl, wl, 4), F) for _ in range(3)]
    src = np.full((hl, wl), NO_SOURCE, np.uint32)
    e = np.asarray(eye, F)
    with np.errstate(all="ignore"):
        d = pos[..., :3] - e
        key = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    key = np.where(np.isnan(key), F(np.inf), key)
    valid = pos[..., 3] != 0
    for Y in range(hl):
        for X in range(wl):
            best, bk = None, None
            for y in range(Y * f, min(Y * f + f, h)):
                for x in range(X * f, min(X * f + f, w)):
                    if valid[y, x] and (best is None or key[y, x] < bk):
                        best, bk = (y, x), key[y, x]
            if best is not None:
                for l, a in zip(lo, (pos, nrm, alb)):
                    l[Y, X] = a[best]
                src[Y, X] = best[0] * w + best[1]
    return lo[0], lo[1], lo[2], src


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _taps(x, y, f, wl, hl, lo_src):
    """The remaining taps of pixel (x, y) in visiting order: [(X, Y, bw)]."""
    X0, wx = tap_weights(x, f)
    Y0, wy = tap_weights(y, f)
    out = []
    for j in (0, 1):
        for i in (0, 1):
            X, Y, bw = X0 + i, Y0 + j, wx[i] * wy[j]
            if X < 0 or X >= wl or Y < 0 or Y >= hl or bw == 0 or lo_src[Y, X] == NO_SOURCE:
                continue
            out.append((X, Y, bw))
    return out


def _blend(taps, lo_plane):
    S, W = None, 0
    with np.errstate(all="ignore"):
        for X, Y, bw in taps:
            v = F(bw) * lo_plane[Y, X]
            S = v if S is None else S + v
            W += bw
        return (S / F(W)).astype(F) if W else None


def upsample(pos, nrm, alb, f, lo_pos, lo_nrm, lo_src, lo_plane, normal_cos=NORMAL_COS, plane_eps=0.0,
             max_holes=0, prefill=None):
    """-> dict: plane [h][w][4] (listed holes keep `prefill`, NaN by default), hole_px (every
    hole, row-major), count, listed (= min(count, max_holes)), hole_pos / hole_nrm / hole_alb
    [R][64][4], stats (representatives, interpolated, holes, overflowed), and per pixel `cls`
    (0 background, 1 representative, 2 interpolated, 3 hole), `accepted`, `rejected` and
    `plane_only` (taps the plane test alone rejected)."""
    pos, nrm, alb, lo_pos, lo_nrm, lo_plane = (np.ascontiguousarray(a, F) for a in (pos, nrm, alb, lo_pos, lo_nrm, lo_plane))
    h, w = pos.shape[:2]
    wl, hl = low_size(w, h, f)
    M = max_holes_of(w, h, max_holes)
    R = (M + HOLE_W - 1) // HOLE_W
    plane = np.full((h, w, 4), np.nan, F) if prefill is None else np.array(prefill, F, copy=True)
    cls = np.zeros((h, w), np.int8)
    accepted, rejected, plane_only = (np.zeros((h, w), np.int8) for _ in range(3))
    ncos, eps = F(normal_cos), F(plane_eps)
    holes = []
    hg = [np.zeros((R * HOLE_W, 4), F) for _ in range(3)]
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if not pos[y, x, 3] != 0:
                    plane[y, x] = 0
                    continue
                p = y * w + x
                if lo_src[y // f, x // f] == p:
                    plane[y, x] = lo_plane[y // f, x // f]
                    cls[y, x] = 1
                    continue
                P, N = pos[y, x], nrm[y, x]
                taps = _taps(x, y, f, wl, hl, lo_src)
                ok = []
                for X, Y, bw in taps:
                    Nq, Pq = lo_nrm[Y, X], lo_pos[Y, X]
                    c = _dot3(N, Nq)
                    d = np.abs(_dot3(N, (Pq[0] - P[0], Pq[1] - P[1], Pq[2] - P[2])))
                    if c >= ncos and d <= eps:
                        ok.append((X, Y, bw))
                    else:
                        rejected[y, x] += 1
                        if c >= ncos:
                            plane_only[y, x] += 1
                accepted[y, x] = len(ok)
                if ok:
                    plane[y, x] = _blend(ok, lo_plane)
                    cls[y, x] = 2
                    continue
                cls[y, x] = 3
                k = len(holes)
                holes.append(p)
                if k < M:
                    for g, a in zip(hg, (pos, nrm, alb)):
                        g[k] = a[y, x]
                else:
                    v = _blend(taps, lo_plane)
                    plane[y, x] = v if v is not None else 0
    count = len(holes)
    stats = (int((cls == 1).sum()), int((cls == 2).sum()), count, max(count - M, 0))
    return {"plane": plane, "hole_px": np.asarray(holes, np.uint32), "count": count, "listed": min(count, M),
            "max_holes": M, "hole_pos": hg[0].reshape(R, HOLE_W, 4), "hole_nrm": hg[1].reshape(R, HOLE_W, 4),
            "hole_alb": hg[2].reshape(R, HOLE_W, 4), "stats": stats, "cls": cls, "accepted": accepted,
            "rejected": rejected, "plane_only": plane_only}


def scatter(plane, hole_plane, hole_px, count, max_holes):
    """plane with plane[hole_px[k]] = hole_plane[k] for k < min(count, max_holes)."""
    out = np.array(plane, F, copy=True).reshape(-1, 4)
    hp = np.ascontiguousarray(hole_plane, F).reshape(-1, 4)
    for k in range(min(count, max_holes)):
        out[hole_px[k]] = hp[k]
    return out.reshape(np.shape(plane))


def trace_mixed(gbuffer, full_diffuse, full_spec, steps_px_diffuse, steps_px_spec, params, eye):
    """The frame vct_trace_mixed_device gives, from a full-resolution trace of the same
    G-buffer: K4 is a function of the record, so the low frame's values are the full frame's
    at the representatives and the hole values the full frame's at the holes.
    params: dict(factor, normal_cos, plane_eps, max_holes).
    -> dict(diffuse, spec, cone_steps, up) with `up` the upsample's dict."""
    pos, nrm, alb = gbuffer
    f = params["factor"]
    h, w = np.shape(pos)[:2]
    lo_pos, lo_nrm, lo_alb, lo_src = pick(pos, nrm, alb, eye, f)
    fd = np.ascontiguousarray(full_diffuse, F).reshape(-1, 4)
    sd = np.asarray(steps_px_diffuse).reshape(-1).astype(np.int64)
    has = lo_src != NO_SOURCE
    lo_plane = np.zeros(lo_src.shape + (4,), F)
    lo_plane[has] = fd[lo_src[has]]
    up = upsample(pos, nrm, alb, f, lo_pos, lo_nrm, lo_src, lo_plane, params["normal_cos"], params["plane_eps"],
                  params.get("max_holes", 0))
    listed = up["hole_px"][:up["listed"]]
    hole_plane = np.zeros((up["hole_pos"].shape[0] * HOLE_W, 4), F)
    hole_plane[:len(listed)] = fd[listed]
    diffuse = scatter(up["plane"], hole_plane, up["hole_px"], up["count"], up["max_holes"])
    steps = int(sd[lo_src[has]].sum()) + int(sd[listed].sum()) + int(np.asarray(steps_px_spec).astype(np.int64).sum())
    return {"diffuse": diffuse, "spec": np.ascontiguousarray(full_spec, F), "cone_steps": steps, "up": up}


def coverage(up, pos):
    """Class shares over the valid pixels of an upsample."""
    valid = np.asarray(pos)[..., 3] != 0
    nv = int(valid.sum())
    cls, acc, rej = up["cls"], up["accepted"], up["rejected"]
    interp = cls == 2
    share = lambda m: float((m & valid).sum()) / max(nv, 1)
    return {"valid": nv, "representatives": share(cls == 1), "one_tap": share(interp & (acc == 1)),
            "multi_tap": share(interp & (acc >= 2)), "mixed": share(interp & (rej >= 1)), "holes": share(cls == 3),
            "plane_only": share(up["plane_only"] >= 1)}


def check_coverage(cov, f):
    """The floors of the shared frames: holes >= 1 % at f = 2 and >= 5 % at f = 4, every other
    class >= 4 %, and at least one tap rejected by the plane test alone."""
    assert cov["valid"] > 0
    assert cov["holes"] >= (0.01 if f == 2 else 0.05), (f, cov)
    for k in ("representatives", "one_tap", "multi_tap", "mixed"):
        assert cov[k] >= 0.04, (f, k, cov)
    assert cov["plane_only"] > 0, (f, cov)
