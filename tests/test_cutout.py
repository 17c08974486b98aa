"""The cutout reference itself (tests/cutout_ref.py) on the CPU: against the oracle where the
mask cannot matter or removes whole triangles, by hand on the threshold cases, and the frame's
independence of the candidate order.  tests/test_cutout_gpu.py holds the HIP path to it."""
import os

import numpy as np
import pytest

import cutout_inputs as CI
import cutout_ref as CR
import gbuffer_ref as GR
import spec_ref as SR

F = np.float32
CASES = {c.name: c for c in CI.all_cases()}
K1 = [n for n, c in CASES.items() if c.k1]
FRAMES = [n for n, c in CASES.items() if c.cam is not None]


def test_binding_declares_the_header():
    """The four calls of include/vct_cutout.h are exported and bound; VctCutout is 16 bytes."""
    import ctypes as C
    from vct import VctCutout, _lib
    lib = _lib.load()
    assert C.sizeof(VctCutout) == 16
    assert _lib.CUTOUT_EXTENSIONS == ("vct_voxelize_cutout", "vct_voxelize_cutout_device", "vct_gbuffer_cutout_device",
                                      "vct_cutout_materials")
    for name in _lib.CUTOUT_EXTENSIONS:
        assert _lib.bind_cutout_extension(lib, name) is not None
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vct_cutout.h")).read()
    for name in _lib.CUTOUT_EXTENSIONS:
        assert name + "(" in header
    assert lib.vct_cutout_materials(None) == 0


def test_mask_sample_is_the_diffuse_formula():
    """M_c is spec_ref.tex_sample on channel c (r, g, b), and the array form equals the scalar
    one in every bit, hostile coordinates included."""
    rng = np.random.default_rng(2)
    u = np.concatenate([rng.uniform(-3, 3, 300), [0.0, 1.0, -1.0, 0.5, np.nan, np.inf, -np.inf, -1e-9, 1e9, 0.25, 0.75]]).astype(F)
    v = np.concatenate([rng.uniform(-3, 3, 300), [1.0, 0.0, 0.5, -2.0, 0.3, np.nan, 0.1, 1e-9, -1e9, 0.5, 0.5]]).astype(F)
    for t in (CI.NOISE, CI.CHANNELS, CI.DIFFUSE, CI.TWO, CI.ONE, CI.STRIPES):
        for k in range(u.size):
            rgb = SR.tex_sample(t, float(u[k]), float(v[k]))
            for c in range(3):
                assert F(CR.mask_scalar(t, float(u[k]), float(v[k]), c)).view(np.uint32) == F(rgb[c]).view(np.uint32)
        for c in range(4):
            want = np.array([CR.mask_scalar(t, float(a), float(b), c) for a, b in zip(u, v)], F)
            assert np.array_equal(CR.mask_sample(t, u, v, c).view(np.uint32), want.view(np.uint32)), c


def test_threshold_values_by_hand():
    """The two-texel mask between its texel centres is M = 2u - 0.5, exact in float32; the 1 x 1
    mask is its texel everywhere."""
    half_dn = float(np.nextafter(F(0.5), F(0)))
    assert CR.mask_scalar(CI.TWO, 0.5, 0.5, 1) == 0.5
    assert CR.mask_scalar(CI.TWO, half_dn, 0.5, 1) == 0.5 - 2.0 ** -24
    assert CR.mask_scalar(CI.TWO, 0.75, 0.5, 0) == 1.0 and CR.mask_scalar(CI.TWO, 0.25, 0.5, 0) == 0.0
    assert bool(CR.covered(CI.TWO, F(0.5), F(0.5), 1, 0.5)) and not bool(CR.covered(CI.TWO, F(half_dn), F(0.5), 1, 0.5))
    assert not bool(CR.covered(CI.TWO, F(0.5), F(0.5), 1, np.nextafter(F(0.5), F(1))))
    for u, v in ((0.0, 0.0), (-3.25, 7.5), (123.4, -0.001), (np.nan, np.inf)):
        assert F(CR.mask_scalar(CI.ONE, u, v, 2)) == CI.M_ONE
    assert bool(CR.covered(CI.ONES, F(0.3), F(0.9), 3, 1.0))           # M == 1.0f exactly: covered at cutoff 1


@pytest.mark.parametrize("name", [n for n in K1 if CASES[n].identity or CASES[n].covered is not None])
def test_k1_equals_oracle_where_the_mask_is_all_or_nothing(oracle_mod, name):
    """Where every point of the masked triangles is covered (or the table is opaque / NULL) the
    sums and counts are oracle.voxelize's of the same mesh; where none is, of the mesh without
    the masked triangles: bit for bit."""
    case = CASES[name]
    sums, counts, rejected = CR.case_k1(case)
    dropped = case.identity == "dropped" or case.covered is False
    v, i, m, kd, mm = case.mesh.without_masked() if dropped else case.mesh.arrays()[:5]
    want = oracle_mod.voxelize(case.n, CI.G0, CI.E, v, i, m, kd, mm, case.textures)
    assert np.array_equal(sums, want[0]) and np.array_equal(counts, want[1]), name
    assert (rejected == 0) == (not dropped) and rejected >= case.min_rejected


@pytest.mark.parametrize("name", K1)
def test_k1_catalogue_shows_what_it_is_about(name):
    case = CASES[name]
    sums, counts, rejected = CR.case_k1(case)
    assert rejected >= case.min_rejected, (name, rejected)
    assert not sums[counts == 0].any()
    if name == "k1_pairs":
        v, i, m, kd, mm, cuts = case.mesh.arrays()
        solid = CR.voxelize(case.n, CI.G0, CI.E, v, i, m, kd, mm, None, case.textures)
        gone = (solid[1] > 0) & (counts == 0)                # every pair rejected: unoccupied
        part = (counts > 0) & (counts < solid[1])            # a rejected and an accepted pair
        assert gone.sum() >= 8 and part.sum() >= 8, (int(gone.sum()), int(part.sum()))
        first = CR.voxelize(case.n, CI.G0, CI.E, v, i[:6], m[:2], kd, mm, cuts, case.textures)
        both = CR.voxelize(case.n, CI.G0, CI.E, v, i[:6], m[:2], kd, mm, None, case.textures)
        assert ((both[1] == 2) & (first[1] == 1)).sum() >= 4  # the diagonal: one of two pairs


def _zeroed(case):
    """The frame of the mesh with the masked triangles' records zeroed (indices preserved)."""
    v, i, m, kd4, mm, _ = case.mesh.arrays()
    rec = GR.k1_skip(GR.tri_records(v, i), v, i, case.n, CI.G0, CI.E)
    rec[[k for k, c in enumerate(case.mesh.cut_of) if c is not None]] = 0
    hit, best, d = GR.nearest_hit(rec, case.cam, case.w, case.h)
    uv = v[i.astype(np.int64).reshape(-1, 3)][..., 6:8].reshape(-1, 6)
    tex_of = None if mm is None else np.asarray(mm, np.int64)[m]
    return hit, GR.planes(rec, kd4[m][:, :3], case.cam, case.w, case.h, CI.ROUGH, hit, best, d, tex_of=tex_of, uv=uv,
                          textures=case.textures, oracle=CR._Spec)


@pytest.mark.parametrize("name", [n for n in FRAMES if CASES[n].identity or CASES[n].covered is not None])
def test_frame_equals_gbuffer_ref_where_the_mask_is_all_or_nothing(name):
    case = CASES[name]
    got = CR.case_frame(case, shaded=False)
    if case.identity == "dropped" or case.covered is False:
        hit, want = _zeroed(case)
    else:
        solid = CR.case_frame(case, shaded=False, solid=True)
        hit, want = solid["hit"], (solid["pos"], solid["nrm"], solid["alb"])
    assert np.array_equal(got["hit"], hit)
    for k, w in zip(("pos", "nrm", "alb"), want):
        assert np.array_equal(got[k].view(np.uint32), w.view(np.uint32)), (name, k)


@pytest.mark.parametrize("name", FRAMES)
def test_frame_does_not_depend_on_the_candidate_order(name):
    """A shuffled visiting order with the same winner rule gives the same winners and t."""
    case = CASES[name]
    v, i, m, _, _, cuts = case.mesh.arrays(case.table)
    mk = CR.masks(cuts, m, i.size // 3)
    rec = GR.k1_skip(GR.tri_records(v, i), v, i, case.n, CI.G0, CI.E)
    uv = v[i.astype(np.int64).reshape(-1, 3)][..., 6:8].reshape(-1, 6)
    n_tex = case.n_tex_after
    a = CR.nearest_hit(rec, case.cam, case.w, case.h, uv, mk, case.textures, n_tex)
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation(rec.shape[0])
        b = CR.nearest_hit(rec, case.cam, case.w, case.h, uv, mk, case.textures, n_tex, order=order)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (name, seed)


@pytest.mark.parametrize("name", FRAMES)
def test_frame_catalogue_shows_what_it_is_about(name):
    case = CASES[name]
    cut, solid = CR.case_frame(case, shaded=False), CR.case_frame(case, shaded=False, solid=True)
    holes = int((cut["hit"] != solid["hit"]).sum())
    assert holes >= case.min_holes, (name, holes)
    if name == "stale_mask":
        assert holes == 0
    if name == "duplicate_coplanar":                      # the higher index wins where the lower is rejected
        n = case.mesh.n_tri
        assert (solid["hit"] == n - 2).sum() >= 10 and np.array_equal(cut["hit"] == n - 1, solid["hit"] == n - 2)
    if name == "near_plane":                              # accepted: background; rejected: the wall
        bg = cut["pos"][..., 3] == 0
        assert (bg & (cut["hit"] >= 2)).sum() >= 100 and ((cut["hit"] < 2) & (solid["hit"] >= 2) & ~bg).sum() >= 100
    if name == "nested":                                  # all three layers are seen
        for lo, hi in ((0, 2), (2, 4), (4, 6)):
            assert ((cut["hit"] >= lo) & (cut["hit"] < hi)).sum() >= 40
    if name == "dynamic_layer":                           # the layer's triangles, in front and through the holes
        n = case.mesh.n_tri
        assert (cut["hit"] == n).sum() >= 20 and (cut["hit"] == n + 1).sum() > (solid["hit"] == n + 1).sum()
    if name == "stack600_masked":                         # winners in all three staging chunks
        for lo, hi in ((0, 100), (100, 256), (256, 512), (512, 600)):
            assert ((cut["hit"] >= lo) & (cut["hit"] < hi)).any(), (lo, hi)


@pytest.mark.parametrize("name", list(CI.ILLEGAL_TABLES))
def test_table_rule(name):
    e = CI.illegal_entry(name, 2)
    bad = CR.table_error([e, CI.OPAQUE] if e else [], 2, n_mat=None if e else 0)
    assert bad is not None
    assert CR.table_error([(1, 3, 1.0, 0), (-1, 0, 0.5, 0)], 2) is None
    assert CR.table_error(None, 0) is None
