"""Hostile G-buffer pixels for K4 (TEST INFRASTRUCTURE): a deterministic catalogue of pixels
that are legal at the ABI (include/vct.h: any pos4.w != 0 is a valid pixel) but lie outside
every family the other parity tests draw from, written over chosen pixels of a clean frame,
and the apertures that exercise the specular step-table cache.

The oracle (vo_trace) defines the result of every entry; the tests compare bit for bit.

Families and entries (`catalogue`):
  position   pos_{x,y,z}{+,-}_{half,3h,far}: outside the grid by 0.5 h, 3 h, 1e3 E, normal = the
             inward axis normal; o0_{x,z} / on_{x,z}: cone origin exactly 0 / exactly n on that
             axis (the inside test is inclusive); pos_big{+,-}: one component +-1e30;
             pos_denorm: x = g0.x + 1e-40 (binary32 sum), y = 1e-40
  posw       w_negzero (-0.0: background), w_two, w_negone, w_nan, w_denorm (1e-45): valid
  normal     n_zero, n_y_negzero (0,1,-0), n_y_poszero (0,1,+0), n_negz (0,0,-1), n_posz (0,0,1),
             n_half / n_four / n_tiny: the pixel's unit normal times 0.5 / 4 / 1e-20
  roughness  r_nan, r_posinf, r_neginf, r_negone, r_zero, r_taumin, r_taumin_prev,
             r_taumin_next, r_one, r_one_next, r_five
  nonfinite  p_posinf_x, p_neginf_y, p_nan_{x,y,z}; n_nan_{x,y,z}, n_posinf_y, n_neginf_z
The eye cases are properties of a frame (`eye_on_pixel`, `EYE_FAR`).

Lane mapping (k4_trace, screen order): a wave is an aligned 8x8 pixel block, lane j at
(mx, my) with mx = bits 0, 2, 4 and my = bits 1, 3, 5 of j (Morton order).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import spec_ref

F = np.float32
FAMILIES = ("position", "posw", "normal", "roughness", "nonfinite")
EYE_FAR = (1e20, 0.0, 0.0)       # v.v overflows binary32
Entry = namedtuple("Entry", "name family apply")     # apply(P, N, A): edits float32[4] rows in place
Frame = namedtuple("Frame", "pos nrm alb entry names where full_block mixed_block isolated")


def lane_of(x: int, y: int) -> int:
    mx, my = x & 7, y & 7
    return (mx & 1) | (my & 1) << 1 | (mx & 2) << 1 | (my & 2) << 2 | (mx & 4) << 2 | (my & 4) << 3


def lane_xy(j: int):
    return (j & 1) | ((j >> 1) & 2) | ((j >> 2) & 4), ((j >> 1) & 1) | ((j >> 2) & 2) | ((j >> 3) & 4)


def cone_origin(P, N, g0, E, n):
    """o = (P - g0) / h + n in the kernels' binary32 operation order (numpy float32)."""
    inv_h = F(n) / F(E)
    with np.errstate(all="ignore"):
        return (np.asarray(P, F)[:3] - np.asarray(g0, F)) * inv_h + np.asarray(N, F)[:3]


def _exact_origin(g0a, E, n, target, na):
    """(P_a, n_a): a position one voxel outside the grid face and the axis normal's component
    (na up to a few ulps: (P_a - g0_a) / h is rarely an integer in binary32) whose cone
    origin v + n_a on that axis is exactly `target`; n_a = target - v is exact (Sterbenz)."""
    inv_h = F(n) / F(E)
    p = F(F(g0a) + F(target - na) * (F(E) / F(n)))
    v = F(F(p - F(g0a)) * inv_h)
    nc = F(F(target) - v)
    assert v + nc == F(target) and abs(float(nc) - na) < 1e-5, (v, nc)
    return p, nc


def catalogue(g0, E, n):
    """-> list of Entry for the grid (g0, E, n)."""
    g0 = np.asarray(g0, F)
    E = F(E)
    h = E / F(n)
    out = []

    def add(name, family, fn):
        out.append(Entry(name, family, fn))

    def set_pos(a, value, normal=None):
        def fn(P, N, A):
            P[a] = value
            if normal is not None:
                N[:3] = normal
        return fn

    axis = np.eye(3, dtype=F)
    for a, an in enumerate("xyz"):
        for s, sn in ((1, "+"), (-1, "-")):
            for dist, dn in ((F(0.5) * h, "half"), (F(3) * h, "3h"), (F(1e3) * E, "far")):
                v = g0[a] + E + dist if s > 0 else g0[a] - dist
                add(f"pos_{an}{sn}_{dn}", "position", set_pos(a, F(v), -s * axis[a]))
    for a, an in ((0, "x"), (2, "z")):
        p0, n0 = _exact_origin(g0[a], E, n, 0.0, 1.0)
        pn, nn = _exact_origin(g0[a], E, n, float(n), -1.0)
        add(f"o0_{an}", "position", set_pos(a, p0, n0 * axis[a]))
        add(f"on_{an}", "position", set_pos(a, pn, nn * axis[a]))
    add("pos_big+", "position", set_pos(0, F(1e30)))
    add("pos_big-", "position", set_pos(1, F(-1e30)))

    def denorm(P, N, A):
        P[0] = g0[0] + F(1e-40)
        P[1] = F(1e-40)
    add("pos_denorm", "position", denorm)

    def set_w(v):
        def fn(P, N, A):
            P[3] = v
        return fn
    for name, v in (("w_negzero", F(-0.0)), ("w_two", F(2)), ("w_negone", F(-1)), ("w_nan", F(np.nan)),
                    ("w_denorm", F(1e-45))):
        add(name, "posw", set_w(v))

    def set_n(v):
        def fn(P, N, A):
            N[:3] = v
        return fn

    def scale_n(s):
        def fn(P, N, A):
            N[:3] = N[:3] * F(s)
        return fn
    add("n_zero", "normal", set_n(np.array([0, 0, 0], F)))
    add("n_y_negzero", "normal", set_n(np.array([0, 1, -0.0], F)))
    add("n_y_poszero", "normal", set_n(np.array([0, 1, 0.0], F)))
    add("n_negz", "normal", set_n(np.array([0, 0, -1], F)))
    add("n_posz", "normal", set_n(np.array([0, 0, 1], F)))
    add("n_half", "normal", scale_n(0.5))
    add("n_four", "normal", scale_n(4.0))
    add("n_tiny", "normal", scale_n(1e-20))

    def set_r(v):
        def fn(P, N, A):
            A[3] = v
        return fn
    tmin = F(spec_ref.TAU_MIN)
    for name, v in (("r_nan", np.nan), ("r_posinf", np.inf), ("r_neginf", -np.inf), ("r_negone", -1.0),
                    ("r_zero", 0.0), ("r_taumin", tmin), ("r_taumin_prev", np.nextafter(tmin, F(0))),
                    ("r_taumin_next", np.nextafter(tmin, F(1))), ("r_one", 1.0),
                    ("r_one_next", np.nextafter(F(1), F(2))), ("r_five", 5.0)):
        add(name, "roughness", set_r(F(v)))

    add("p_posinf_x", "nonfinite", set_pos(0, F(np.inf)))
    add("p_neginf_y", "nonfinite", set_pos(1, F(-np.inf)))
    for a, an in enumerate("xyz"):
        add(f"p_nan_{an}", "nonfinite", set_pos(a, F(np.nan)))

    def set_nc(a, v):
        def fn(P, N, A):
            N[a] = v
        return fn
    for a, an in enumerate("xyz"):
        add(f"n_nan_{an}", "nonfinite", set_nc(a, F(np.nan)))
    add("n_posinf_y", "nonfinite", set_nc(1, F(np.inf)))
    add("n_neginf_z", "nonfinite", set_nc(2, F(-np.inf)))
    return out


def build(clean, g0, E, n, families=FAMILIES, keep_clean_blocks=8, exclude=()):
    """Writes the catalogue entries of `families` over pixels of the clean (pos, nrm, alb) frame.

    Layout, in the order of the frame's 8x8 blocks sorted by their number of valid clean pixels:
    one block hostile in all 64 pixels (the entries in turn), one block mixing one entry of
    each of at least three families when that many are selected, then one block per entry with
    the entry at lane 0 and every other pixel as in the clean frame, while more than
    `keep_clean_blocks` blocks remain untouched (`exclude`: entry names left out).  A hostile pixel edits the clean pixel it
    replaces, or the frame's donor pixel (the valid pixel nearest the centre) over background.
    -> Frame; `entry` is the catalogue index per pixel (-1 clean), `isolated` the names placed
    in a block of their own.  The placement conditions are asserted here."""
    pos, nrm, alb = (np.array(a, F, copy=True) for a in clean)
    hh, ww = pos.shape[:2]
    assert hh % 8 == 0 and ww % 8 == 0
    cat = catalogue(g0, E, n)
    sel = [i for i, e in enumerate(cat) if e.family in families and e.name not in exclude]
    valid0 = clean[0][..., 3] != 0
    ys, xs = np.nonzero(valid0)
    d = np.argmin((ys - hh // 2) ** 2 + (xs - ww // 2) ** 2)
    donor = tuple(np.array(a[ys[d], xs[d]], F) for a in clean)
    blocks = sorted(((by, bx) for by in range(hh // 8) for bx in range(ww // 8)),
                    key=lambda b: (-int(valid0[b[0] * 8:b[0] * 8 + 8, b[1] * 8:b[1] * 8 + 8].sum()), b))
    entry = np.full((hh, ww), -1, np.int32)
    where = []

    def put(i, y, x):
        src = clean if valid0[y, x] else None
        P, N, A = (np.array(a[y, x], F) for a in src) if src else (v.copy() for v in donor)
        with np.errstate(all="ignore"):
            cat[i].apply(P, N, A)
        pos[y, x], nrm[y, x], alb[y, x] = P, N, A
        entry[y, x] = i
        where.append((cat[i].name, y, x))

    it = iter(blocks)
    full = next(it)
    for j in range(64):
        mx, my = lane_xy(j)
        put(sel[j % len(sel)], full[0] * 8 + my, full[1] * 8 + mx)
    mixed = None
    fams = [f for f in FAMILIES if f in families]
    if len(fams) >= 3:
        mixed = next(it)
        for j, f in enumerate(fams):
            i = next(i for i in sel if cat[i].family == f and cat[i].name != "w_negzero")
            mx, my = lane_xy(5 * j + 1)
            put(i, mixed[0] * 8 + my, mixed[1] * 8 + mx)
    rest = list(it)
    isolated = []
    for i, b in zip(sel, rest[:max(len(rest) - keep_clean_blocks, 0)]):
        put(i, b[0] * 8, b[1] * 8)
        isolated.append(cat[i].name)
    fr = Frame(pos, nrm, alb, entry, [e.name for e in cat], where, full, mixed, isolated)

    # ---- placement conditions -------------------------------------------------
    hostile = entry >= 0
    blk = lambda b: (slice(b[0] * 8, b[0] * 8 + 8), slice(b[1] * 8, b[1] * 8 + 8))
    assert hostile[blk(full)].all()
    assert {cat[i].name for i in sel} <= {w[0] for w in where}, "every selected entry is placed"
    if mixed is not None:
        assert len({cat[i].family for i in entry[blk(mixed)].ravel() if i >= 0}) >= 3
    valid = pos[..., 3] != 0
    for name in isolated:
        y, x = next((y, x) for nm, y, x in where if nm == name and (y // 8, x // 8) not in (full, mixed))
        b = blk((y // 8, x // 8))
        assert hostile[b].sum() == 1, name                      # the block's other pixels are clean
        if name != "w_negzero":                                 # (a background entry is no valid lane)
            lanes = [lane_of(xx, yy) for yy in range(8) for xx in range(8) if valid[b][yy, xx]]
            assert valid[y, x] and lane_of(x, y) == min(lanes), name   # the wave's lowest valid lane
    assert 4 * int((hostile & valid).sum()) <= int(valid.sum()), "hostile pixels: at most a quarter"
    untouched = sum(1 for b in blocks if not hostile[blk(b)].any())
    assert untouched >= min(keep_clean_blocks, len(blocks) - 2)
    for a, c in zip((pos, nrm, alb), clean):
        assert np.array_equal(a[~hostile].view(np.uint32), np.asarray(c, F)[~hostile].view(np.uint32))
    return fr


def eye_on_pixel(clean):
    """An eye bit-equal to the position of the valid pixel nearest the frame's centre (vl = 0)."""
    valid = clean[0][..., 3] != 0
    ys, xs = np.nonzero(valid)
    hh, ww = valid.shape
    d = np.argmin((ys - hh // 2) ** 2 + (xs - ww // 2) ** 2)
    return tuple(float(v) for v in clean[0][ys[d], xs[d], :3]), (int(ys[d]), int(xs[d]))


def bits_equal(got, ref):
    """Bit-exact comparison of a trace result dict with the oracle's: float outputs through a
    uint32 view, step counts as integers.  -> list of the keys that differ."""
    bad = []
    for key in ("diffuse", "spec"):
        if not np.array_equal(np.ascontiguousarray(got[key], F).view(np.uint32),
                              np.ascontiguousarray(ref[key], F).view(np.uint32)):
            bad.append(key)
    if got.get("steps_px") is not None and not np.array_equal(np.asarray(got["steps_px"]).astype(np.uint32),
                                                               ref["steps_px"]):
        bad.append("steps_px")
    if got.get("cone_steps") is not None and int(got["cone_steps"]) != int(ref["cone_steps"]):
        bad.append("cone_steps")
    return bad


def describe_diff(got, ref, frame=None):
    """Names the pixels (and their catalogue entries) where got differs from ref."""
    d = np.zeros(ref["steps_px"].shape, bool)
    for key in ("diffuse", "spec"):
        d |= (np.ascontiguousarray(got[key], F).view(np.uint32) !=
              np.ascontiguousarray(ref[key], F).view(np.uint32)).any(-1)
    if got.get("steps_px") is not None:
        d |= np.asarray(got["steps_px"]).astype(np.uint32) != ref["steps_px"]
    ys, xs = np.nonzero(d)
    names = [(int(y), int(x), frame.names[frame.entry[y, x]] if frame is not None and frame.entry[y, x] >= 0
              else "clean") for y, x in zip(ys[:12], xs[:12])]
    return f"{int(d.sum())} pixels differ, first: {names}"


def check_reference(ref, ref_clean, frame, clean):
    """Conditions on the oracle alone, so a comparison with it cannot pass vacuously."""
    for key in ("diffuse", "spec"):
        assert np.isfinite(ref[key]).all(), f"oracle {key} not finite"
    hostile = frame.entry >= 0
    cv = (clean[0][..., 3] != 0) & ~hostile
    assert (ref["steps_px"][cv] != 0).mean() >= 0.9, "clean valid pixels with steps"
    for key in ("diffuse", "spec"):        # the oracle is per pixel: this checks the builder
        assert np.array_equal(ref[key][~hostile].view(np.uint32), ref_clean[key][~hostile].view(np.uint32)), key
    assert np.array_equal(ref["steps_px"][~hostile], ref_clean["steps_px"][~hostile])
    neg = [(y, x) for nm, y, x in frame.where if nm == "w_negzero"]
    for y, x in neg:                       # -0.0 is background: all zeros, no steps
        assert not ref["diffuse"][y, x].view(np.uint32).any() and not ref["spec"][y, x].view(np.uint32).any()
        assert ref["steps_px"][y, x] == 0


# ---------------------------------------------------------------------------
# specular step tables: apertures by step count
# ---------------------------------------------------------------------------
def spec_steps(tau, n):
    """Steps of an unobstructed specular march: t = 1; D = max(1, 2 tau t); t += 0.5 D while
    t <= n sqrt3, in binary32 (tau clamped as the spec does)."""
    tau = np.fmin(np.fmax(F(tau), F(spec_ref.TAU_MIN)), F(spec_ref.TAU_MAX))
    tau2, tmax, t, k = F(2) * tau, F(n) * F(spec_ref.SQRT3), F(1), 0
    while t <= tmax:
        D = np.fmax(F(1), tau2 * t)
        t = t + F(0.5) * D
        k += 1
    return k


def tau_with_steps(steps, n):
    """The largest binary32 aperture whose unobstructed march at grid size n takes `steps`
    steps (the count does not increase with tau), by bisection over the bit patterns."""
    lo, hi = F(spec_ref.TAU_MIN).view(np.uint32), F(spec_ref.TAU_MAX).view(np.uint32)
    f = lambda b: spec_steps(np.uint32(b).view(F), n)
    assert f(lo) >= steps >= f(hi)
    lo, hi = int(lo), int(hi)
    while hi - lo > 1:                     # invariant: f(lo) >= steps; hi: f(hi) < steps or the top
        mid = (lo + hi) // 2
        if f(mid) >= steps:
            lo = mid
        else:
            hi = mid
    tau = np.uint32(lo).view(F)
    assert spec_steps(tau, n) == steps, (steps, spec_steps(tau, n))
    return float(tau)


def aperture_sets(n):
    """Two disjoint sets of 12 roughness values for a grid of size n (more than kSpecSlots = 8
    table keys each).  The first holds 0.02, the 63-, 64- and 65-step apertures, 1.0, two
    values below TAU_MIN and two above TAU_MAX (they clamp onto the keys of TAU_MIN / TAU_MAX)."""
    t63, t64, t65 = (tau_with_steps(k, n) for k in (63, 64, 65))
    first = [0.02, t63, t64, t65, 1.0, 0.001, -3.0, 2.5, 40.0, 0.1, 0.25, 0.5]
    second = [0.03, 0.045, 0.06, 0.08, 0.12, 0.15, 0.2, 0.3, 0.4, 0.6, 0.75, 0.9]
    first, second = [float(F(v)) for v in first], [float(F(v)) for v in second]
    assert len(set(first)) == 12 and len(set(second)) == 12 and not set(first) & set(second)
    return first, second


def block_roughness(alb, values, shift=0):
    """A copy of alb with one roughness per 8x8 block, cycling through `values`."""
    out = np.array(alb, F, copy=True)
    hh, ww = out.shape[:2]
    for by in range(hh // 8):
        for bx in range(ww // 8):
            out[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8, 3] = values[(by * (ww // 8) + bx + shift) % len(values)]
    return out
