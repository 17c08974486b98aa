"""numpy restatement of include/vct_spec.h "temporal accumulation" (include/vct_temporal.h).
Every float operation is a float32 numpy operation in the spec's order, so the GPU kernel is
compared with it bit for bit: planes, lengths and stats.
"""
import numpy as np

from fog_ref import _tanf

F = np.float32
NORMAL_COS = F(0.9)
DEFAULT_LEN, MAX_LEN = 8, 1024
# per-pixel classes of accumulate()'s `cls`
BACKGROUND, REUSED, OFFSCREEN, REJECTED = 0, 1, 2, 3
# and the reset causes of its `cause` (0: not a reset)
NO_CAMERA, NO_MOTION, PROJECTION, NO_TAP, NON_FINITE, LENGTH_ONE = 1, 2, 3, 4, 5, 6


def camera_constants(cam, w, h):
    """The host constants of vct_view.h camera_fields for a vct.camera.Camera or a VctCamera:
    dict(eye, front, right, up [3] float32, tan_half, aspect)."""
    c = cam.to_ctypes() if hasattr(cam, "to_ctypes") else cam
    v = lambda a: np.array([a[0], a[1], a[2]], F)
    return {"eye": v(c.position), "front": v(c.front), "right": v(c.right), "up": v(c.up),
            "tan_half": _tanf(F(c.zoom_deg) * F(0.5) * F(3.14159265358979) / F(180.0)), "aspect": F(w) / F(h)}


def check_camera(cam, w=4, h=3):
    """The input rule of prev_cam: None, or what is wrong."""
    k = camera_constants(cam, w, h)
    if not (np.isfinite(k["tan_half"]) and k["tan_half"] > 0):
        return "tan(zoom / 2) is not finite and > 0"
    if not all(np.isfinite(k[n]).all() for n in ("eye", "front", "right", "up")):
        return "non-finite position or vector"
    return None


def check_params(normal_cos, plane_eps, max_len):
    """The params' input rule: None, or what is wrong."""
    nc, pe = F(normal_cos), F(plane_eps)
    if not np.isfinite(nc) or nc < -1 or nc > 1:
        return "normal_cos outside [-1, 1]"
    if not np.isfinite(pe) or np.signbit(pe):
        return "plane_eps not finite or negative"
    if not 1 <= int(max_len) <= MAX_LEN:
        return "max_len outside 1 .. 1024"
    return None


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def project(q, cam, w, h):
    """Last frame's pixel coordinates of the points q [..., 3]: (fx, fy, ok) with ok = every
    projection test passed (z > 0, -1 < fx < w, -1 < fy < h)."""
    k = camera_constants(cam, w, h)
    q = np.ascontiguousarray(q, F)
    with np.errstate(all="ignore"):
        v = q - k["eye"]
        z, a, b = _dot3(v, k["front"]), _dot3(v, k["right"]), _dot3(v, k["up"])
        kx = k["tan_half"] * k["aspect"]
        sx, sy = a / (z * kx), b / (z * k["tan_half"])
        fx = ((sx + F(1.0)) * F(0.5)) * F(w) - F(0.5)
        fy = ((F(1.0) - sy) * F(0.5)) * F(h) - F(0.5)
        ok = (z > 0) & (fx > F(-1.0)) & (fx < F(w)) & (fy > F(-1.0)) & (fy < F(h))
    return fx.astype(F), fy.astype(F), ok


def tap_weights(f):
    """-> (x0, (weight of tap x0, weight of tap x0 + 1)) for a checked coordinate f."""
    X16 = int(np.floor(F(f) * F(16.0) + F(0.5)))
    x0, r = X16 >> 4, X16 & 15
    return x0, (16 - r, r)


def accumulate(pos, nrm, cur, prev_cam=None, prev_pos=None, prev_nrm=None, hist=None, hist_len=None, motion=None,
               normal_cos=NORMAL_COS, plane_eps=0.0, max_len=DEFAULT_LEN):
    """cur / hist: sequences of n_planes [h][w][4] planes.  -> dict: out (list of planes),
    out_len [h][w] uint32, stats (valid, reused, reset_offscreen, reset_rejected), and per
    pixel `cls` (BACKGROUND, REUSED, OFFSCREEN, REJECTED), `cause` (why it reset), `accepted`
    (taps), `rejected` (taps the tests refused), `weights` (distinct bw among the accepted
    taps), `edge` (a tap index of -1, w or h) and `taps` ({(y, x): [(Y, X, bw) accepted]})."""
    assert check_params(normal_cos, plane_eps, max_len) is None
    pos, nrm = np.ascontiguousarray(pos, F), np.ascontiguousarray(nrm, F)
    cur = [np.ascontiguousarray(c, F) for c in cur]
    h, w = pos.shape[:2]
    NP = len(cur)
    out = [np.zeros((h, w, 4), F) for _ in range(NP)]
    out_len = np.zeros((h, w), np.uint32)
    cls, cause = np.zeros((h, w), np.int8), np.zeros((h, w), np.int8)
    accepted, rejected, weights = (np.zeros((h, w), np.int8) for _ in range(3))
    edge = np.zeros((h, w), bool)
    taps = {}
    ncos, eps = F(normal_cos), F(plane_eps)
    valid = pos[..., 3] != 0
    proj = np.zeros((h, w), bool)
    cause[valid] = NO_CAMERA
    if prev_cam is not None:
        assert check_camera(prev_cam, w, h) is None
        prev_pos, prev_nrm = np.ascontiguousarray(prev_pos, F), np.ascontiguousarray(prev_nrm, F)
        hist = [np.ascontiguousarray(a, F) for a in hist]
        hist_len = np.ascontiguousarray(hist_len).astype(np.uint32)
        q = pos[..., :3] if motion is None else np.ascontiguousarray(motion, F)[..., :3]
        fx, fy, proj = project(q, prev_cam, w, h)
        cause[valid] = PROJECTION
        if motion is not None:
            gone = np.ascontiguousarray(motion, F)[..., 3] == 0
            cause[valid & gone] = NO_MOTION
            proj = proj & ~gone
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if not valid[y, x]:
                    continue
                c = OFFSCREEN
                if proj[y, x]:
                    c = REJECTED
                    N, qq = nrm[y, x], q[y, x]
                    x0, wx = tap_weights(fx[y, x])
                    y0, wy = tap_weights(fy[y, x])
                    edge[y, x] = x0 < 0 or x0 + 1 >= w or y0 < 0 or y0 + 1 >= h
                    S, W, L, seen = None, 0, None, set()
                    for j in (0, 1):
                        for i in (0, 1):
                            X, Y, bw = x0 + i, y0 + j, wx[i] * wy[j]
                            if X < 0 or X >= w or Y < 0 or Y >= h or bw == 0:
                                continue
                            Pq, lq = prev_pos[Y, X], int(hist_len[Y, X])
                            if Pq[3] == 0 or lq == 0:
                                continue
                            cn = _dot3(N, prev_nrm[Y, X])
                            d = np.abs(_dot3(N, Pq[:3] - qq))
                            if not (cn >= ncos and d <= eps):
                                rejected[y, x] += 1
                                continue
                            fb = F(bw)
                            v = [fb * hp[Y, X] for hp in hist]
                            S = v if S is None else [s + t for s, t in zip(S, v)]
                            W += bw
                            L = lq if L is None else min(L, lq)
                            seen.add(bw)
                            accepted[y, x] += 1
                            taps.setdefault((y, x), []).append((Y, X, bw))
                    weights[y, x] = len(seen)
                    cause[y, x] = NO_TAP
                    if W:
                        H = [(s / F(W)).astype(F) for s in S]
                        k = min(L, max_len - 1) + 1
                        cause[y, x] = LENGTH_ONE if k < 2 else NON_FINITE
                        if all(np.isfinite(a).all() for a in H) and k >= 2:
                            c = REUSED
                            cause[y, x] = 0
                            wk = F(1.0) / F(k)
                            for p in range(NP):
                                out[p][y, x] = H[p] + (cur[p][y, x] - H[p]) * wk
                            out_len[y, x] = k
                if c != REUSED:
                    for p in range(NP):
                        out[p][y, x] = cur[p][y, x]
                    out_len[y, x] = 1
                cls[y, x] = c
    n = lambda v: int((cls == v).sum())
    stats = (int(valid.sum()), n(REUSED), n(OFFSCREEN), n(REJECTED))
    assert stats[0] == sum(stats[1:])
    return {"out": out, "out_len": out_len, "stats": stats, "cls": cls, "cause": cause, "taps": taps, "accepted": accepted, "rejected": rejected,
            "weights": weights, "edge": edge}


def coverage(r):
    """Shares over the valid pixels of an accumulate() result, and the counts the moved-camera
    frame must show."""
    cls = r["cls"]
    nv = max(int((cls != BACKGROUND).sum()), 1)
    reused = cls == REUSED
    return {"valid": int((cls != BACKGROUND).sum()),
            "multi_weight": float((reused & (r["accepted"] >= 2) & (r["weights"] >= 2)).sum()) / nv,
            "offscreen": int((cls == OFFSCREEN).sum()), "rejected": int((cls == REJECTED).sum()),
            "mixed": int((reused & (r["rejected"] >= 1)).sum()), "edge": int(r["edge"].sum())}


def check_moved_coverage(cov):
    """The floors of the moved-camera frame (the issue's list)."""
    assert cov["valid"] > 0
    assert cov["multi_weight"] >= 0.25, cov
    for k in ("offscreen", "rejected", "mixed", "edge"):
        assert cov[k] >= 1, (k, cov)
