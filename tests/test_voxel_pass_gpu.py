"""K1, the dynamic layer and the emission grid run one conservative voxelization pass
(csrc/vct_voxel_sat.h: triangle setup, candidate walk, SAT).  One mesh that stresses what they
share goes through all three, each in its host and its device form, and each result is
compared bit for bit with the CPU oracle's voxelization of that mesh.
"""
import numpy as np
import pytest

import emission_ref

pytestmark = pytest.mark.gpu

F = np.float32
N, G0, EXTENT = 16, (0.0, 0.0, 0.0), 16.0     # h = 1: q is the vertex itself


def walk_mesh():
    """-> (verts [V, 3], idx, tri_material, kd4 = ke4 = 1), candidates per triangle.
    Zero-candidate triangles first, in the middle and last; one triangle whose candidate box is the
    whole grid (16^3 = 4096 candidates: buckets 0..7 of 512 all start in it); one-voxel slivers;
    4123 candidates in all, a multiple of neither 8 nor 2 (the last lane of each walk is partial)."""
    nan = np.nan
    tris = [
        ([-10, -10, -10], [-9, -10, -10], [-10, -9, -10], 0),          # outside the grid
        ([-2, -2, -2], [18, 18, 7], [7, 18, 18], 4096),                # spans it
        ([3.2, 4.2, 5.2], [3.4, 4.2, 5.2], [3.2, 4.4, 5.3], 1),        # a sliver in voxel (3, 4, 5)
        ([2.5, 2.5, 2.5], [nan, 3.5, 2.5], [2.5, 3.5, 3.5], 0),        # a NaN vertex: skipped
        ([10.6, 2.1, 13.3], [10.8, 2.2, 13.3], [10.6, 2.3, 13.5], 1),  # a sliver in voxel (10, 2, 13)
        ([7.9, 8.2, 8.2], [8.1, 8.2, 8.2], [7.9, 8.4, 8.3], 2),        # a sliver across a voxel face
        ([5.5, 5.5, 5.5], [5.5, 5.5, 5.5], [5.5, 5.5, 5.5], 1),        # degenerate, inside: a hit with a zero normal
        ([1.5, 1.5, 12.5], [5.5, 1.7, 12.5], [1.5, 4.5, 12.6], 20),    # 5 x 4 x 1
        ([3.3, 4.5, 5.6], [3.7, 4.5, 5.6], [3.3, 4.8, 5.7], 1),        # second hits of the two sliver voxels
        ([10.2, 2.6, 13.6], [10.4, 2.7, 13.6], [10.2, 2.8, 13.8], 1),
        ([20, 20, 20], [20, 20, 20], [20, 20, 20], 0),                 # degenerate and outside
    ]
    verts = np.array([p for t in tris for p in t[:3]], F)
    idx = np.arange(verts.shape[0], dtype=np.uint32)
    return (verts, idx, np.zeros(len(tris), np.uint32), np.ones((1, 4), F)), [t[3] for t in tris]


def candidate_counts(verts, n):
    """vct_spec.h "K1 input rule" restated: per triangle the candidate count, 0 for a non-finite q.
    (h = 1 and g0 = 0 here, so q is the vertex.)"""
    out = []
    for q in np.asarray(verts, F).reshape(-1, 3, 3):
        if not np.isfinite(q).all():
            out.append(0)
            continue
        cnt = 1
        for a in range(3):
            top = F(n) + F(1)
            lo = max(int(np.ceil(min(max(q[:, a].min(), F(-1)), top))) - 1, 0)
            hi = min(int(np.floor(max(min(q[:, a].max(), top), F(-1)))), n - 1)
            cnt *= max(hi - lo + 1, 0)
        out.append(cnt)
    return out


def _dev(a, t):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()


def test_three_passes_agree_with_the_oracle(gpu_ready, oracle_mod):
    import torch
    from vct import Context
    (v, i, m, k), cand = walk_mesh()
    assert candidate_counts(v, N) == cand
    total, offs = sum(cand), np.concatenate([[0], np.cumsum(cand)])
    assert total % 8 != 0 and total % 2 != 0                               # both walks end in a partial lane
    assert cand[0] == 0 and cand[-1] == 0 and 0 in cand[2:-1]              # no candidates: first, last, in between
    assert all(offs[1] <= 512 * b < offs[2] for b in range(8))             # eight bucket starts inside triangle 1
    assert cand.count(1) >= 3
    sums, counts = oracle_mod.voxelize(N, G0, EXTENT, v, i, m, k)
    ao, nm = oracle_mod.resolve(N, sums, counts)
    occupied = int((counts > 0).sum())
    print("occupied voxels", occupied, "hits", int(counts.sum()))
    assert occupied > 100 and counts.reshape(N, N, N)[5, 4, 3] == 2 and counts.reshape(N, N, N)[5, 5, 5] >= 1
    em = emission_ref.emission(oracle_mod, N, G0, EXTENT, counts, v, i, m, k)
    assert np.array_equal(em["emissive"].reshape(-1), counts > 0) and em["dropped"] == 0

    def assert_grid(ctx, what):
        got_sums, got_counts = ctx.download_accum()
        assert np.array_equal(got_counts, counts), f"{what}: counts"
        assert np.array_equal(got_sums, sums), f"{what}: sums"
        got_ao, got_nm = ctx.download_voxels()
        assert emission_ref.bits_equal(got_ao, ao) and emission_ref.bits_equal(got_nm, nm), f"{what}: voxels"

    ctx = Context(N, G0, EXTENT)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dv, di, dm, dk = _dev(v, F), _dev(i, np.int32), _dev(m, np.int32), _dev(k, F)
    empty = (np.zeros((0, 3), F), np.zeros(0, np.uint32))
    for form in ("host", "device"):
        # 1. K1
        if form == "host":
            ctx.voxelize(v, i, m, k)
        else:
            ctx.voxelize_device(dv, di, dm, dk)
        assert_grid(ctx, f"voxelize, {form}")
        # 3. the emission grid over it: Ke = 1 everywhere, so every occupied voxel emits
        if form == "host":
            ctx.voxelize_emission(v, i, m, k)
        else:
            ctx.voxelize_emission_device(dv, di, dm, dk)
        assert emission_ref.bits_equal(ctx.download_emission(), em["E"]), f"emission, {form}"
        assert ctx.emission_voxels() == occupied
        # 2. the same triangles as a layer over an empty static grid
        ctx.voxelize(*empty)
        assert not ctx.download_accum()[1].any()
        if form == "host":
            ctx.voxelize_dynamic(v, i, m, k)
        else:
            ctx.voxelize_dynamic_device(dv, di, dm, dk)
        assert_grid(ctx, f"voxelize_dynamic, {form}")
        assert ctx.dynamic_voxels() == occupied
    ctx.close()
