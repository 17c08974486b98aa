"""Reference for include/vct_emission.h (TEST INFRASTRUCTURE ONLY).

The CPU oracle needs no emission of its own: the emission grid is a composition of its
calls (vct_spec.h "emissive surfaces") --

    sums_e, _ = oracle.voxelize(n, g0, E, emitter_verts, emitter_idx, tri_material, ke4)
    E_grid    = oracle.resolve(n, sums_e, counts_of_K1)[0][..., :3]     where counts_of_K1 > 0

(K1's own sums of Ke in place of Kd, divided by K1's hit counts of the voxelized mesh), and
the rest is float32 numpy in the spec's order: level 0 = K2 + scale * E, the pixel lookup,
and a composite = another composite's output + scale * Em.
"""
from __future__ import annotations

import numpy as np

F = np.float32
LAMP_KD = (0.78, 0.78, 0.78)
LAMP_KE = (17.0, 12.0, 4.0)
FLOATING = [(0.0, 0.3, 0.5), (0.3, 0.3, 0.5), (0.0, 0.5, 0.7)]     # a triangle in the room's empty air
SOUP_KE = [(3.0, 1.0, 0.5), (0.0, 0.0, 0.0), (0.25, 0.25, 8.0), (1.0, 2.0, 0.0)]


def bits_equal(a, b) -> bool:
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def lamp_scene():
    """scenes.cornell() with the skylight hole filled by an emissive quad of its own material.
    -> (scene, ke4 [materials, 4], the lamp's material index)"""
    from vct import scenes
    s = scenes.cornell()
    lamp = s.material(LAMP_KD)
    s.rect_y(1.0, -0.5, 0.5, -0.5, 0.5, -1, lamp)
    ke = np.zeros((len(s.kd), 4), F)
    ke[lamp, :3] = LAMP_KE
    return s, ke, lamp


def emission(O, n, g0, E, counts_k1, verts, idx, tri_material, ke4):
    """The emission grid of emitter triangles over a voxelization with hit counts counts_k1
    [n^3].  -> dict(E [n, n, n, 4] float32 as vct_download_emission gives it, emissive
    [n, n, n] bool, hits [n^3]: per voxel the SAT hits of the triangles whose Ke is not zero,
    dropped: voxels with such a hit that the voxelization left empty)."""
    ke4 = np.ascontiguousarray(ke4, F).reshape(-1, 4)
    idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
    mat = np.zeros(idx.size // 3, np.uint32) if tri_material is None else np.asarray(tri_material, np.uint32)
    sums, _ = O.voxelize(n, g0, E, verts, idx, mat, ke4)
    ao, _ = O.resolve(n, sums, counts_k1)
    occ = (np.asarray(counts_k1) > 0).reshape(n, n, n)
    emissive = occ & np.any(sums[:, :3] != 0, axis=1).reshape(n, n, n)
    out = np.zeros((n, n, n, 4), F)
    out[emissive, :3] = ao[emissive, :3]
    out[emissive, 3] = 1.0
    # the hits of the emitting triangles alone (the oracle counts a zero-Ke triangle's too)
    glow = np.flatnonzero(np.any(ke4[mat, :3] != 0, axis=1))
    hits = np.zeros(n ** 3, np.uint32)
    if glow.size:
        _, hits = O.voxelize(n, g0, E, verts, idx.reshape(-1, 3)[glow].reshape(-1), mat[glow], ke4)
    assert np.array_equal(hits.reshape(n, n, n)[occ] > 0, emissive[occ])       # Ke >= 0: no sum cancels
    return {"E": out, "emissive": emissive, "hits": hits, "dropped": int(((hits > 0) & ~occ.reshape(-1)).sum())}


def classes(em, counts_k1):
    """Coverage classes of an emission grid: emissive voxels, those every triangle of which
    emits (only), those shared with triangles that do not (mixed), those with >= 2 emitting hits."""
    e = em["emissive"].reshape(-1)
    hits, cnt = em["hits"], np.asarray(counts_k1)
    return {"emissive": int(e.sum()), "only": int((e & (hits == cnt)).sum()), "mixed": int((e & (hits < cnt)).sum()),
            "multi": int((e & (hits >= 2)).sum()), "dropped": em["dropped"]}


def add_to_level0(r0, E_grid, scale=1.0):
    """Level 0 after vct_inject_emission: L.c = L.c + (scale * E.c) at the emissive voxels."""
    out = np.array(r0, F, copy=True)
    em = E_grid[..., 3] != 0
    with np.errstate(all="ignore"):
        out[em, :3] = out[em, :3] + F(scale) * E_grid[em, :3]
    return out


def lookup(n, g0, E, E_grid, pos4):
    """Em [h, w, 3] of a G-buffer's positions and the mask of the pixels that land in an
    emissive voxel: p = (P - g0) * inv_h, used iff 0 <= p_c < n in float32 on all axes."""
    pos4 = np.asarray(pos4, F)
    inv_h = F(n) / F(E)
    with np.errstate(all="ignore"):
        p = (pos4[..., :3] - np.asarray(g0, F)) * inv_h
        inside = np.all((p >= F(0.0)) & (p < F(n)), axis=-1) & (pos4[..., 3] != 0)
        v = np.where(inside[..., None], np.floor(p), 0).astype(np.int64)
    cell = E_grid[v[..., 2], v[..., 1], v[..., 0]]
    hit = inside & (cell[..., 3] != 0)
    Em = np.where(hit[..., None], cell[..., :3], F(0.0)).astype(F)
    return Em, hit


def composite(base, pos4, Em, scale=1.0):
    """vct_composite_emissive_device from the linear output `base` of the composite without
    the term (lights_ref.composite: vis NULL; shadow_ref.composite: a vis plane)."""
    out = np.array(base, F, copy=True)
    fg = np.asarray(pos4, F)[..., 3] != 0
    with np.errstate(all="ignore"):
        out[fg, :3] = out[fg, :3] + F(scale) * Em[fg]
    return out


def hostile_ke(n_tri):
    """Ke of the hostile catalogue's triangle t (one material each): float32((t % 5 + 1) / 4) x
    (1, 0.5, 0.25), zero for every third triangle."""
    ke = np.zeros((n_tri, 4), F)
    for t in range(n_tri):
        if t % 3 != 2:
            ke[t, :3] = F((t % 5 + 1) / 4) * np.array([1.0, 0.5, 0.25], F)
    return ke


_lamp = {}


def lamp(n):
    """The lamp scene at n^3 on the CPU oracle, computed once (treat as read-only): scene,
    arrays, ke, g0, E, grid (oracle.pipeline's dict, lit by scenes.LIGHT_DIR), em (the emission
    grid of the whole mesh with the lamp's Ke), classes."""
    if n not in _lamp:
        from oracle import oracle as O
        from vct import scenes
        O.build()
        s, ke, lamp_mat = lamp_scene()
        arrays = s.arrays()
        g0, E = scenes.grid_for_unit_box(n)
        grid = O.pipeline(n, g0, E, *arrays, scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
        em = emission(O, n, g0, E, grid["counts"], arrays[0], arrays[1], arrays[2], ke)
        for a in (grid["albedo_occ"], grid["normal"], grid["r0"], grid["counts"], em["E"], em["emissive"]):
            a.setflags(write=False)
        _lamp[n] = {"scene": s, "arrays": arrays, "ke": ke, "lamp": lamp_mat, "g0": g0, "E": E, "grid": grid,
                    "em": em, "classes": classes(em, grid["counts"])}
    return _lamp[n]
