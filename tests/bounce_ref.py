"""Reference of vct_inject_bounces (include/vct_spec.h "light bounces"), test infrastructure.

The CPU oracle has no bounce of its own and needs none: `vo_trace` accepts any G-buffer,
so the expected grid is a composition of oracle calls.  The source G-buffer is built in
float32 numpy exactly as the spec writes it, `oracle.trace(..., specular=False)` gathers,
`L0 + A * I` is applied in float32 (one multiply, one add) and `oracle.build_mips`
rebuilds the pyramid.  Every comparison against it is bit-exact.

Grids are (n, n, n, 4) float32 indexed [z][y][x] (linear-Z, as they cross the ABI).
"""
from __future__ import annotations

import functools

import numpy as np


def sources(ao: np.ndarray, nm: np.ndarray):
    """(z, y, x) index arrays of the sources -- occupied voxels with a nonzero normal --
    in linear-Z order, and those of the occupied voxels with a zero normal."""
    occ = ao[..., 3] != 0
    has_n = np.any(nm[..., :3] != 0, axis=-1)
    return np.nonzero(occ & has_n), np.nonzero(occ & ~has_n)


def source_gbuffer(n, g0, E, ao, nm):
    """The sources as a 1 x S G-buffer (pos4, nrm4, alb4) and their (z, y, x) indices."""
    (z, y, x), _ = sources(ao, nm)
    g0 = np.asarray(g0, np.float32)
    hh = np.float32(E) / np.float32(n)                       # float divide
    S = x.size
    pos = np.zeros((1, S, 4), np.float32)
    for c, idx in enumerate((x, y, z)):
        pos[0, :, c] = g0[c] + (idx.astype(np.float32) + np.float32(0.5)) * hh   # multiply, then add
    pos[0, :, 3] = 1.0
    nrm = np.zeros((1, S, 4), np.float32)
    nrm[0, :, :3] = nm[z, y, x, :3]
    alb = np.zeros((1, S, 4), np.float32)
    alb[0, :, :3] = ao[z, y, x, :3]
    assert pos.dtype == np.float32
    return (pos, nrm, alb), (z, y, x)


def gather(O, n, g0, E, level0, pyr, gbuf, aniso, n_diffuse):
    """I = K4.diffuse.rgb at every source, [S, 3] float32, and the cone steps taken."""
    pos, nrm, alb = gbuf
    if n_diffuse == 0 or pos.shape[1] == 0:
        return np.zeros((pos.shape[1], 3), np.float32), 0
    out = O.trace(n, g0, E, level0, pyr, pos, nrm, alb, (0.0, 0.0, 0.0), aniso=aniso, n_diffuse=n_diffuse,
                  specular=False)
    return out["diffuse"][0, :, :3].copy(), out["cone_steps"]


def bounce(O, n, g0, E, ao, nm, r0, n_bounces, aniso=True, n_diffuse=9):
    """-> list over k = 0..n_bounces of dict(level0, pyr, I, steps): entry 0 is the input
    (I, steps = None), entry k the grid after k bounces, I / steps the gather that made it."""
    r0 = np.ascontiguousarray(r0, np.float32)
    gbuf, (z, y, x) = source_gbuffer(n, g0, E, ao, nm)
    A = ao[z, y, x, :3].astype(np.float32)
    out = [{"level0": r0, "pyr": O.build_mips(n, r0, aniso), "I": None, "steps": None}]
    for _ in range(n_bounces):
        cur = out[-1]
        I, steps = gather(O, n, g0, E, cur["level0"], cur["pyr"], gbuf, aniso, n_diffuse)
        nxt = r0.copy()                                      # every bounce adds to L0 (Jacobi)
        prod = A * I
        nxt[z, y, x, :3] = r0[z, y, x, :3] + prod            # float32: one multiply, one add
        assert nxt.dtype == np.float32 and prod.dtype == np.float32
        out.append({"level0": nxt, "pyr": O.build_mips(n, nxt, aniso), "I": I, "steps": steps})
    return out


def reference(O, n, g0, E, arrays, light, color=(1.0, 1.0, 1.0), aniso=True, n_diffuse=9, n_bounces=2):
    """K1 -> K2 -> K3 on the oracle, then n_bounces bounces -> (oracle.pipeline dict, bounce list)."""
    v, i, m, k = arrays
    grid = O.pipeline(n, g0, E, v, i, m, k, light, color, aniso=aniso)
    return grid, bounce(O, n, g0, E, grid["albedo_occ"], grid["normal"], grid["r0"], n_bounces, aniso, n_diffuse)


@functools.lru_cache(maxsize=None)
def cornell(n=32, aniso=True, n_diffuse=9, n_bounces=2, light=None):
    """The shared Cornell reference (computed once per configuration; treat as read-only):
    dict(grid = oracle.pipeline(...), bounces = bounce(...), g0, E, arrays)."""
    from oracle import oracle as O
    from vct import scenes
    O.build()
    s = scenes.cornell()
    v, i, m, k = s.arrays()
    g0, E = scenes.grid_for_unit_box(n)
    grid, b = reference(O, n, g0, E, (v, i, m, k), light or scenes.LIGHT_DIR, scenes.LIGHT_COLOR, aniso, n_diffuse,
                        n_bounces)
    return {"grid": grid, "bounces": b, "g0": g0, "E": E, "arrays": (v, i, m, k), "scene": s}


def pyramid_equal(ctx, pyr_flat) -> bool:
    """Every face of levels 1..L of a vct.Context against the oracle's flat pyramid, bit for bit."""
    from helpers import gpu_pyramid_flat
    got = gpu_pyramid_flat(ctx)
    return got.shape == pyr_flat.shape and np.array_equal(got.view(np.uint32), pyr_flat.view(np.uint32))


def bits_equal(a, b) -> bool:
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
