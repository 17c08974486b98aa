"""K1 on the hostile-triangle catalogue (tests/voxel_inputs.py) against the CPU oracle, bit for
bit: one test per family (a difference names its family), the exact-arithmetic band checked
directly against the GPU's counts, the entry points and the context's state across calls, the
n_tri shapes of the list-building kernels, the Kd error rule, and the G-buffer passes over
skipped triangles.  tests/test_voxel_inputs.py checks the reference itself on the CPU."""
import numpy as np
import pytest

import voxel_inputs as VI
from helpers import gpu_pyramid_flat

pytestmark = pytest.mark.gpu
F = np.float32
GRIDS = [(n, pl) for n in (8, 16) for pl in VI.PLACEMENTS]
LIGHTS = ("scene", (1.0, 1.0, 1.0))
_cache = {}


def _light(l):
    from vct import scenes
    return scenes.LIGHT_DIR if l == "scene" else l


def _ref(O, mesh, key=None):
    """The oracle's K1 of the mesh and, per light, its level 0 and pyramid (computed once per key)."""
    if key is not None and key in _cache:
        return _cache[key]
    sums, counts = O.voxelize(mesh.n, mesh.g0, mesh.E, mesh.verts, mesh.idx, mesh.mat, mesh.kd)
    ao, nm = O.resolve(mesh.n, sums, counts)
    lit = {}
    for l in LIGHTS:
        r0 = O.inject(mesh.n, ao, nm, _light(l))
        lit[l] = (r0, O.build_mips(mesh.n, r0, True))
    ref = dict(sums=sums, counts=counts, ao=ao, nm=nm, lit=lit)
    if key is not None:
        _cache[key] = ref
    return ref


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _check(ctx, mesh, ref, what, lights=LIGHTS):
    """download_accum and download_voxels equal the oracle; then K2 + K3 per light do."""
    got = ctx.download_accum()
    assert np.array_equal(got[0], ref["sums"]) and np.array_equal(got[1], ref["counts"]), \
        f"{what}: " + VI.describe_diff(got, (ref["sums"], ref["counts"]), mesh)
    ao, nm = ctx.download_voxels()
    assert np.array_equal(_bits(ao), _bits(ref["ao"])), f"{what}: albedo / occupancy"
    assert np.array_equal(_bits(nm), _bits(ref["nm"])), f"{what}: normals"
    for l in lights:
        ctx.inject_directional(_light(l))
        ctx.build_mips()
        r0, pyr = ref["lit"][l]
        assert np.array_equal(_bits(ctx.download_level(0)), _bits(r0)), f"{what}: level 0, light {l}"
        assert np.array_equal(_bits(gpu_pyramid_flat(ctx)), _bits(pyr)), f"{what}: pyramid, light {l}"


def _voxelize(ctx, mesh):
    ctx.voxelize(mesh.verts, mesh.idx, mesh.mat, mesh.kd)


def _ctx(mesh, **kw):
    from vct import Context
    return Context(mesh.n, mesh.g0, mesh.E, **kw)


def _run(O, mesh, what, key=None):
    ref = _ref(O, mesh, key)
    ctx = _ctx(mesh)
    _voxelize(ctx, mesh)
    _check(ctx, mesh, ref, what)
    ctx.close()
    return ref


# ---------------------------------------------------------------------------
# one test per family
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,pl", GRIDS)
def test_family_lattice(gpu_ready, oracle_mod, n, pl):
    ref = _run(oracle_mod, VI.build(("lattice",), n, pl), "lattice")
    assert ref["counts"].sum() > 100


@pytest.mark.parametrize("n,pl", GRIDS)
def test_family_degenerate(gpu_ready, oracle_mod, n, pl):
    """Points, segments and a zero-normal triangle: zero-normal voxels go through K2 and K3."""
    ref = _run(oracle_mod, VI.build(("degenerate",), n, pl), "degenerate")
    occ = ref["ao"][..., 3] != 0
    assert occ.sum() >= 8 and (~ref["nm"][occ][:, :3].any(-1)).sum() >= 8      # occupied, normal (0, 0, 0)


@pytest.mark.parametrize("n,pl", GRIDS)
def test_family_sliver(gpu_ready, oracle_mod, n, pl):
    ref = _run(oracle_mod, VI.build(("sliver",), n, pl), "sliver / tiny / giant")
    assert ref["counts"].sum() > n * n


@pytest.mark.parametrize("n,pl", GRIDS)
def test_family_outside(gpu_ready, oracle_mod, n, pl):
    mesh = VI.build(("outside",), n, pl)
    ref = _run(oracle_mod, mesh, "outside")
    assert 6 <= ref["counts"].sum() <= 64                    # the straddling and touching entries only
    none = VI.build(("outside", "nonfinite"), n, pl, only_kind=("none",))      # every triangle without candidates
    ref = _run(oracle_mod, none, "all outside")
    assert not ref["counts"].any()


@pytest.mark.parametrize("n,pl", GRIDS)
def test_family_nonfinite(gpu_ready, oracle_mod, n, pl):
    """Skipped triangles leak nothing: the grid equals the oracle's, which equals (CPU test) the
    grid of the clean neighbours alone."""
    mesh = VI.build(("nonfinite",), n, pl)
    ref = _run(oracle_mod, mesh, "nonfinite")
    clean = _ref(oracle_mod, VI.build(("nonfinite",), n, pl, only_kind=("clean",)))
    assert np.array_equal(ref["sums"], clean["sums"]) and ref["counts"].sum() == 30


@pytest.mark.parametrize("n,pl", GRIDS)
def test_family_materials(gpu_ready, oracle_mod, n, pl):
    """With Kd = 32767.99 in the mesh K1 takes the seven-atomic path; without it the packed
    one, where the mixed-sign voxel's low halves borrow from the high ones."""
    ref = _run(oracle_mod, VI.build(("materials",), n, pl), "materials (unpacked)")
    assert ref["sums"][:, :3].max() == int(float(F(32767.99)) * 65536) > 2 ** 31 - 1024 and ref["counts"].max() == 12
    mesh = VI.build(("materials",), n, pl, exclude=("kd_max",))
    ref = _run(oracle_mod, mesh, "materials (packed)")
    v = int(np.argmax(ref["counts"]))
    assert ref["sums"][v, 0] < 0 < ref["sums"][v, 1] and ref["sums"][v, 2] < 0


@pytest.mark.parametrize("n,pl", GRIDS)
def test_family_counts(gpu_ready, oracle_mod, n, pl):
    """A giant triangle between one-candidate triangles, 1..9 candidates in a row, and meshes of
    0, 1, 1023, 1024 and 1025 triangles, most of them without candidates."""
    O = oracle_mod
    _run(O, VI.build(("counts",), n, pl), "counts")
    _run(O, VI.empty_mesh(n, pl), "0 triangles")
    for n_tri in (1, 1023, 1024, 1025):
        mesh, expect = VI.count_mesh(n_tri, n, pl)
        ref = _run(O, mesh, f"n_tri = {n_tri}")
        assert np.array_equal(ref["counts"], expect)


def test_counts_big(gpu_ready, oracle_mod):
    """262 152 triangles (257 scan tiles: k_scan_carry's second block; long runs without
    candidates in front of every live triangle, the last one live)."""
    mesh, expect = VI.count_mesh(262145 + 7, 8)
    ref = _ref(oracle_mod, mesh)
    assert np.array_equal(ref["counts"], expect) and expect.sum() == 300
    ctx = _ctx(mesh)
    _voxelize(ctx, mesh)
    _check(ctx, mesh, ref, "n_tri = 262152", lights=LIGHTS[:1])
    ctx.close()


# ---------------------------------------------------------------------------
# the exact-arithmetic band, directly against the GPU's counts
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bands():
    """Per grid: the seeded mesh, the catalogue mesh and their per-voxel inner / outer counts
    in exact integer arithmetic (computed once per module)."""
    out = {}
    for n, pl in GRIDS:
        for name, mesh in (("seeded", VI.seeded_mesh(n, pl)), ("catalogue", VI.build(VI.FAMILIES, n, pl))):
            out[n, pl, name] = (mesh,) + VI.band_counts(mesh)
    return out


@pytest.mark.parametrize("n,pl", GRIDS)
def test_exact_band(gpu_ready, bands, n, pl):
    """Every voxel's count lies between the number of triangles whose exact overlap with the
    box of half-size 0.5 - 2^-14 is certain and the number that overlap the box of half-size
    0.5 + 2^-14: the float32 SAT on the GPU is conservative up to contacts thinner than 2^-14."""
    for name in ("seeded", "catalogue"):
        mesh, lo, hi = bands[n, pl, name]
        assert int(lo.sum()) > 150 and (name == "catalogue" or int(hi.sum()) - int(lo.sum()) <= 0.10 * int(hi.sum()))
        ctx = _ctx(mesh)
        _voxelize(ctx, mesh)
        counts = ctx.download_accum()[1]
        ctx.close()
        missed, extra = np.flatnonzero(counts < lo), np.flatnonzero(counts > hi)
        assert missed.size == 0 and extra.size == 0, \
            f"{name}: counts below the inner set at voxels {missed[:8]}, above the outer set at {extra[:8]}"


# ---------------------------------------------------------------------------
# entry points and state
# ---------------------------------------------------------------------------
def _dev_args(mesh):
    import torch
    dev = torch.device("cuda")
    return (torch.from_numpy(mesh.verts).to(dev), torch.from_numpy(mesh.idx.astype(np.int32)).to(dev),
            torch.from_numpy(mesh.mat.astype(np.int32)).to(dev), torch.from_numpy(mesh.kd).to(dev))


@pytest.mark.parametrize("n,pl", [(8, "exact"), (16, "unit")])
def test_entry_points_and_state(gpu_ready, oracle_mod, tmp_path, n, pl):
    from helpers import scene_arrays
    from vct import dump
    O = oracle_mod
    mesh = VI.build(VI.FAMILIES, n, pl, exclude=("kd_max",))
    ref = _ref(O, mesh, ("all", n, pl))
    _, (v, i, m, k) = scene_arrays("cornell")
    cornell = VI.Mesh(v, i, m, k, None, None, n, mesh.g0, mesh.E, pl)
    cref = _ref(O, cornell, ("cornell", n, pl))

    ctx = _ctx(mesh)
    ctx.voxelize_device(*_dev_args(mesh))                     # the device form
    _check(ctx, mesh, ref, "device entry point")
    _voxelize(ctx, mesh)                                      # the host form, a second identical call
    _check(ctx, mesh, ref, "host entry point, second call")
    _voxelize(ctx, cornell)                                   # sparse reset after a hostile mesh
    _check(ctx, cornell, cref, "cornell after the hostile mesh")
    _voxelize(ctx, mesh)
    _check(ctx, mesh, ref, "the hostile mesh after cornell")
    dump.save_grid(ctx, tmp_path / "g", pyramid=True)         # save -> load round trip
    back = dump.load_grid(tmp_path / "g")
    _check(back, mesh, ref, "loaded dump")
    back.close()
    ctx.close()

    multi = _ctx(mesh, devices=2)                             # a 2-device context equals one device
    _voxelize(multi, mesh)
    _check(multi, mesh, ref, "2-device context")
    multi.close()


# ---------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------
def test_bad_kd(gpu_ready, oracle_mod):
    """NaN, +-Inf and +-32768 in each of Kd's r, g, b through the host and the device entry
    points: VCT_EINVAL with the rule's message, inject / mips / trace then VCT_ESTATE, and a
    clean voxelize on the same context afterwards equals the oracle."""
    import torch
    from vct import VctError
    mesh = VI.build(("materials", "lattice"), 8)
    ref = _ref(oracle_mod, mesh)
    z = np.zeros((2, 2, 4), F)
    ctx = _ctx(mesh)
    for comp in range(3):
        for val in (np.nan, np.inf, -np.inf, 32768.0, -32768.0):
            kd = mesh.kd.copy()
            kd[3, comp] = val
            for form in ("host", "device"):
                _voxelize(ctx, mesh)
                with pytest.raises(VctError, match="EINVAL.*Kd not finite or .Kd. >= 32768"):
                    if form == "host":
                        ctx.voxelize(mesh.verts, mesh.idx, mesh.mat, kd)
                    else:
                        args = _dev_args(mesh)
                        ctx.voxelize_device(*args[:3], torch.from_numpy(kd).to(args[0].device))
                for call in (lambda: ctx.inject_directional((0.0, 1.0, 0.0)), ctx.build_mips,
                             lambda: ctx.trace(z, z, z, (0, 0, 0))):
                    with pytest.raises(VctError, match="ESTATE"):
                        call()
    _voxelize(ctx, mesh)
    _check(ctx, mesh, ref, "clean voxelize after the errors")
    kd = np.concatenate([mesh.kd, np.full((1, 4), np.nan, F)])     # an unused material's Kd is not read
    ctx.voxelize(mesh.verts, mesh.idx, mesh.mat, kd)
    ctx.voxelize_device(*_dev_args(mesh)[:3], torch.from_numpy(kd).cuda())
    _check(ctx, mesh, ref, "unused NaN material", lights=())
    ctx.close()


# ---------------------------------------------------------------------------
# G-buffer passes over skipped triangles
# ---------------------------------------------------------------------------
class _Scene:
    def __init__(self, mesh):
        self.mesh = mesh

    def arrays(self):
        return self.mesh.verts, self.mesh.idx, self.mesh.mat, self.mesh.kd


def test_gbuffer_skips_nonfinite(gpu_ready):
    """vct_gbuffer_raycast_device and vct_gbuffer_raster_device over the non-finite and
    degenerate families (with the lattice family as something to see) at 64 x 48: equal to each
    other and to the passes over the mesh with the skipped entries removed, bit for bit, and to
    scenes.raycast_numpy of that mesh (a binary64 caster: the tolerances of
    test_parity_gpu.py::test_raycast_matches_numpy)."""
    import torch
    from vct import scenes
    from vct.camera import Camera
    n, w, h = 8, 64, 48
    fams = ("nonfinite", "degenerate", "lattice")
    mesh, keep = VI.build(fams, n), VI.build(fams, n, only_kind=("clean", "live"))
    assert len(mesh.names) - len(keep.names) == 30
    cam = Camera(position=(4.0, 4.0, 14.0))
    dev = torch.device("cuda")
    outs = []
    for m in (mesh, keep):
        ctx = _ctx(m)
        _voxelize(ctx, m)
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        for fn in (ctx.gbuffer_raycast_device, ctx.gbuffer_raster_device):
            gb = [torch.full((h, w, 4), 7.0, device=dev) for _ in range(3)]
            fn(cam, w, h, 0.1, *gb)
            torch.cuda.synchronize()
            outs.append([g.cpu().numpy() for g in gb])
        ctx.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert np.array_equal(_bits(a), _bits(b))
    gp, gn, ga = outs[0]
    assert np.isfinite(gp).all() and np.isfinite(gn).all() and np.isfinite(ga).all()
    with np.errstate(all="ignore"):
        rp, rn, ra = scenes.raycast_numpy(_Scene(keep), cam, w, h, 0.1)
    assert (rp[..., 3] > 0).sum() >= 40
    assert (gp[..., 3] == rp[..., 3]).mean() > 0.995
    both = (gp[..., 3] > 0) & (rp[..., 3] > 0)
    assert np.all(np.abs(gn[both] - rn[both]) < 1e-3, axis=-1).mean() > 0.99
    assert np.abs(gp[both][:, :3] - rp[both][:, :3]).max() < 1e-3
    # albedo names the triangle hit: equal except on the diagonal x = y that the two diag_a
    # triangles share (the camera looks down that line's pixels: either triangle is nearest)
    apart = both & (np.abs(rp[..., 0] - rp[..., 1]) > 1e-3)
    assert apart.sum() >= 0.95 * both.sum() and np.array_equal(ga[apart], ra[apart])
