"""The hostile-triangle catalogue (tests/voxel_inputs.py) and its reference, on the CPU:
spec_ref.voxelize against the C oracle over the whole catalogue (bit-exact: the expected values
of the GPU tests rest on two independent restatements), the float32 SAT against exact integer
arithmetic (conservative up to contacts thinner than 2^-14 voxel), the expectations the
catalogue states by construction, the Kd error rule on the oracle and the CPU backend, and the
oracle under -fsanitize=address,undefined,float-cast-overflow on the catalogue (a stand-alone
driver run as a child process)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import spec_ref
import voxel_inputs as VI

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GRIDS = [(n, pl) for n in (8, 16) for pl in VI.PLACEMENTS]
SIZES = {"lattice": 12, "degenerate": 8, "sliver": 6, "outside": 33, "nonfinite": 60, "materials": 16,
         "counts": 12}


def _vox(O, mesh, tris=None):
    """oracle K1 of the mesh (or of the listed triangles only) -> (sums, counts)"""
    idx = mesh.idx if tris is None else mesh.idx.reshape(-1, 3)[list(tris)].ravel()
    mat = mesh.mat if tris is None else mesh.mat[list(tris)]
    return O.voxelize(mesh.n, mesh.g0, mesh.E, mesh.verts, idx, mat, mesh.kd)


def _hits(O, mesh, t):
    return set(np.flatnonzero(_vox(O, mesh, [t])[1]).tolist())


def test_catalogue_entries():
    for n in (8, 16):
        cat = VI.catalogue(n)
        names = [e.name for e in cat]
        assert len(set(names)) == len(names)
        sizes = {f: sum(e.family == f for e in cat) for f in VI.FAMILIES}
        print("catalogue size per family:", sizes)
        assert sizes == SIZES
    a, b = VI.build(VI.FAMILIES, 16, "unit"), VI.build(VI.FAMILIES, 16, "unit")
    assert a.verts.tobytes() == b.verts.tobytes()          # deterministic


@pytest.mark.parametrize("n,pl", GRIDS)
def test_spec_ref_equals_oracle(oracle_mod, n, pl):
    """Both restatements agree over the whole catalogue, sums and counts, and on the small
    n_tri meshes, before any GPU comparison rests on them."""
    mesh = VI.build(VI.FAMILIES, n, pl)
    ref = _vox(oracle_mod, mesh)
    got = spec_ref.voxelize(n, mesh.g0, mesh.E, mesh.verts, mesh.idx, mesh.mat, mesh.kd)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), VI.describe_diff(got, ref, mesh)
    assert ref[1].sum() > 2 * n * n
    for n_tri in (1, 1025):
        m, expect = VI.count_mesh(n_tri, n, pl)
        ref = _vox(oracle_mod, m)
        got = spec_ref.voxelize(n, m.g0, m.E, m.verts, m.idx, m.mat, m.kd)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def _band_check(O, mesh, tris):
    """inner <= hits <= outer per triangle -> (missed, extra, |outer|, |outer - inner|)"""
    q = VI.q_of(mesh.verts, mesh.g0, mesh.E, mesh.n).reshape(-1, 3, 3)
    missed, extra, n_out, n_band = [], [], 0, 0
    for t in tris:
        inner, outer = VI.exact_sets(q[t], mesh.n)
        hits = _hits(O, mesh, t)
        if inner - hits:
            missed.append((mesh.names[t], sorted(inner - hits)[:4]))
        if hits - outer:
            extra.append((mesh.names[t], sorted(hits - outer)[:4]))
        n_out += len(outer)
        n_band += len(outer - inner)
    return missed, extra, n_out, n_band


@pytest.mark.parametrize("n,pl", GRIDS)
def test_exact_band_seeded(oracle_mod, n, pl):
    """400 seeded adversarial triangles: every voxel whose box of half-size 0.5 - 2^-14 overlaps
    in exact arithmetic is hit, every hit voxel overlaps the box of half-size 0.5 + 2^-14; the
    band between the two holds at most 10 % of the outer set (the check is not vacuous)."""
    mesh = VI.seeded_mesh(n, pl)
    assert VI.delta_for(VI.q_of(mesh.verts, mesh.g0, mesh.E, n).reshape(-1, 3, 3)[0], n) == VI.S >> 14
    missed, extra, n_out, n_band = _band_check(oracle_mod, mesh, range(len(mesh.names)))
    print(f"seeded band n={n} {pl}: outer {n_out}, band {n_band} = {100.0 * n_band / n_out:.2f} %")
    assert not missed and not extra, (missed[:5], extra[:5])
    assert n_out > 1000 and n_band <= 0.10 * n_out


@pytest.mark.parametrize("n,pl", GRIDS)
def test_exact_band_catalogue(oracle_mod, n, pl):
    """The same band for every finite entry; degenerate entries against exact point / segment
    sets.  The lattice family is mostly band by design: its share is reported, not capped."""
    mesh = VI.build(VI.FAMILIES, n, pl)
    q = VI.q_of(mesh.verts, mesh.g0, mesh.E, n).reshape(-1, 3, 3)
    fin = [t for t in range(len(mesh.names)) if np.isfinite(q[t]).all()]
    missed, extra, _, _ = _band_check(oracle_mod, mesh, fin)
    assert not missed and not extra, (missed[:5], extra[:5])
    lat = [t for t in fin if mesh.entries[t].family == "lattice"]
    _, _, n_out, n_band = _band_check(oracle_mod, mesh, lat)
    print(f"lattice band n={n} {pl}: outer {n_out}, band {n_band} = {100.0 * n_band / n_out:.2f} %")
    # every degenerate shape is recognised as one (exact sets by point / segment, not the 13 axes)
    kinds = {mesh.names[t]: VI._shape(VI._ints(q[t]))[0] for t in fin if mesh.entries[t].family == "degenerate"}
    assert all(k == "point" for nm, k in kinds.items() if nm.startswith("pt_")), kinds
    if pl == "exact":
        assert kinds["col_axis"] == kinds["col_oblique"] == kinds["two_equal"] == "segment", kinds
        assert kinds["tiny_area"] == "triangle"


def test_exact_arithmetic_known_answers():
    """The integer tests themselves, on cases with closed-form answers."""
    S = VI.S
    half = S // 2
    tri = [[0, 0, S], [4 * S, 0, S], [0, 4 * S, S]]                     # in the plane z = 1
    c = lambda x, y, z: (x * S + half, y * S + half, z * S + half)
    assert VI.exact_overlap(tri, *c(0, 0, 0), half) and VI.exact_overlap(tri, *c(0, 0, 1), half)   # closed: both layers
    assert not VI.exact_overlap(tri, *c(0, 0, 2), half)
    assert not VI.exact_overlap(tri, *c(0, 0, 0), half - 1) and not VI.exact_overlap(tri, *c(0, 0, 1), half - 1)
    assert VI.exact_overlap(tri, *c(0, 0, 0), half + 1) and not VI.exact_overlap(tri, *c(5, 0, 0), half)
    assert VI.exact_overlap(tri, *c(1, 2, 0), half) and not VI.exact_overlap(tri, *c(3, 3, 0), half)   # hypotenuse x + y = 4
    assert VI.exact_overlap(tri, *c(2, 2, 1), half) and not VI.exact_overlap(tri, *c(2, 2, 1), half - 1)  # corner on it
    p = (3 * S, 3 * S, 3 * S)
    assert sum(VI.exact_segment(p, p, *c(x, y, z), half) for x in range(6) for y in range(6) for z in range(6)) == 8
    assert sum(VI.exact_segment(p, p, *c(x, y, z), half - 1) for x in range(6) for y in range(6) for z in range(6)) == 0
    a, b = (half, half, half), (3 * S + half, 3 * S + half, half)       # the diagonal through corners
    hit = {(x, y) for x in range(5) for y in range(5) if VI.exact_segment(a, b, *c(x, y, 0), half)}
    assert hit == {(i, i) for i in range(4)} | {(i, i + 1) for i in range(3)} | {(i + 1, i) for i in range(3)}
    hit = {(x, y) for x in range(5) for y in range(5) if VI.exact_segment(a, b, *c(x, y, 0), half - 1)}
    assert hit == {(i, i) for i in range(4)}


@pytest.mark.parametrize("n,pl", GRIDS)
def test_expectations_by_construction(oracle_mod, n, pl):
    O = oracle_mod
    mesh = VI.build(VI.FAMILIES, n, pl)
    for t, e in enumerate(mesh.entries):
        if e.kind == "none":                                   # outside and non-finite entries add nothing
            s, c = _vox(O, mesh, [t])
            assert not c.any() and not s.any(), e.name
        elif e.hits is not None and pl == "exact":
            s, c = _vox(O, mesh, [t])
            assert c.sum() == e.hits and c.max() == 1, (e.name, int(c.sum()), e.hits)
    # the clean neighbours' voxel sums equal a run without the hostile entries
    full = _vox(O, VI.build(("nonfinite",), n, pl))
    clean = _vox(O, VI.build(("nonfinite",), n, pl, only_kind=("clean",)))
    assert np.array_equal(full[0], clean[0]) and np.array_equal(full[1], clean[1])
    assert clean[1].sum() == 30
    if pl == "exact":                                          # a point on a corner: exactly its 8 voxels
        t = mesh.names.index("pt_corner")
        want = {x + n * (y + n * z) for x in (5, 6) for y in (5, 6) for z in (5, 6)}
        assert _hits(O, mesh, t) == want
    # zero normal: the tiny_area entry adds no normal, so its voxel resolves to a zero normal
    s, c = _vox(O, mesh, [mesh.names.index("tiny_area")])
    assert c.sum() >= 1 and not s[:, 3:].any()
    # counts family
    e = VI.empty_mesh(n, pl)
    s, c = O.voxelize(n, e.g0, e.E, e.verts, e.idx, e.mat, e.kd)
    assert not c.any() and not s.any()
    out = VI.build(("outside", "nonfinite"), n, pl, only_kind=("none",))
    assert len(out.names) == 55 and not _vox(O, out)[1].any()              # all triangles outside: total 0
    for n_tri in (1, 1023, 1024, 1025):
        m, expect = VI.count_mesh(n_tri, n, pl)
        assert np.array_equal(_vox(O, m)[1], expect) and expect.sum() >= min(n_tri, 10)


def test_count_mesh_big(oracle_mod):
    """262 152 triangles (257 scan tiles: k_scan_carry's second block), 300 of them live."""
    m, expect = VI.count_mesh(262145 + 7, 8)
    assert expect.sum() == 300 and m.idx.size == 3 * 262152
    assert np.array_equal(_vox(oracle_mod, m)[1], expect)


BAD_KD = [(c, v) for c in range(3) for v in (np.nan, np.inf, -np.inf, 32768.0, -32768.0)]


@pytest.fixture(scope="module")
def cpu_lib(oracle_mod):
    import ctypes as C
    from vct import _lib
    return _lib.bind(C.CDLL(oracle_mod.CPU_BACKEND))


def test_bad_kd_is_refused(oracle_mod, cpu_lib):
    """NaN, +-Inf and +-32768 in each of Kd's r, g, b: the oracle returns its error code, the CPU
    backend VCT_EINVAL with the rule's message, and the grid is refused afterwards (VCT_ESTATE);
    the largest legal magnitude just below passes."""
    from vct import Context, VctError, scenes
    mesh = VI.build(("materials",), 8)
    z = np.zeros((2, 2, 4), F)
    for comp, val in BAD_KD:
        kd = mesh.kd.copy()
        kd[3, comp] = val
        with pytest.raises(ValueError, match="Kd"):
            oracle_mod.voxelize(8, mesh.g0, mesh.E, mesh.verts, mesh.idx, mesh.mat, kd)
        with pytest.raises(ValueError, match="Kd"):
            spec_ref.voxelize(8, mesh.g0, mesh.E, mesh.verts, mesh.idx, mesh.mat, kd)
        ctx = Context(8, mesh.g0, mesh.E, lib=cpu_lib)
        ctx.voxelize(mesh.verts, mesh.idx, mesh.mat, mesh.kd)
        with pytest.raises(VctError, match="EINVAL.*Kd not finite") as ei:
            ctx.voxelize(mesh.verts, mesh.idx, mesh.mat, kd)
        assert ei.value.status == 1
        for call in (lambda: ctx.inject_directional(scenes.LIGHT_DIR), ctx.build_mips,
                     lambda: ctx.trace(z, z, z, (0, 0, 0))):
            with pytest.raises(VctError, match="ESTATE"):
                call()
        ctx.voxelize(mesh.verts, mesh.idx, mesh.mat, mesh.kd)
        ref = oracle_mod.voxelize(8, mesh.g0, mesh.E, mesh.verts, mesh.idx, mesh.mat, mesh.kd)
        got = ctx.download_accum()
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        ctx.close()
    kd = mesh.kd.copy()
    kd[0, :3] = np.nextafter(F(32768), F(0))
    kd[1, :3] = -np.nextafter(F(32768), F(0))
    s, c = oracle_mod.voxelize(8, mesh.g0, mesh.E, mesh.verts, mesh.idx, mesh.mat, kd)
    assert s[:, :3].max() == 2 ** 31 - 128 and s[:, :3].min() == -(2 ** 31 - 128)
    # an unused material's Kd is not read
    kd = np.concatenate([mesh.kd, np.full((1, 4), np.nan, F)])
    oracle_mod.voxelize(8, mesh.g0, mesh.E, mesh.verts, mesh.idx, mesh.mat, kd)


def test_cpu_backend_skips_nonfinite_triangles(oracle_mod, cpu_lib):
    """The CPU backend over the non-finite family: the oracle's grid, and G-buffer passes that
    equal the mesh with the skipped entries removed."""
    from vct import Context
    from vct.camera import Camera
    n = 8
    mesh = VI.build(("nonfinite", "degenerate", "lattice"), n)
    keep = VI.build(("nonfinite", "degenerate", "lattice"), n, only_kind=("clean", "live"))
    ref = _vox(oracle_mod, mesh)
    cam = Camera(position=(4.0, 4.0, 14.0))
    w, h = 64, 48
    outs = []
    for m in (mesh, keep):
        ctx = Context(n, m.g0, m.E, lib=cpu_lib)
        ctx.voxelize(m.verts, m.idx, m.mat, m.kd)
        got = ctx.download_accum()
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        bufs = [np.full((h, w, 4), 7.0, F) for _ in range(3)]
        ctx.gbuffer_raycast_device(cam, w, h, 0.1, *[b.ctypes.data for b in bufs])
        outs.append(bufs)
        ctx.close()
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (outs[0][0][..., 3] != 0).sum() >= 5


# ---------------------------------------------------------------------------
# the oracle under sanitizers on the whole catalogue
# ---------------------------------------------------------------------------
def test_oracle_voxelize_under_sanitizers(oracle_mod, tmp_path):
    """oracle/vct_oracle.c built with -fsanitize=address,undefined,float-cast-overflow runs
    vo_voxelize and vo_resolve over the whole catalogue (both grids, both placements) and over a
    bad-Kd mesh in a child process: no report, and the same bits as the oracle library."""
    probe = subprocess.run(["gcc", "-fsanitize=address,undefined,float-cast-overflow", "-x", "c", "-", "-o",
                            str(tmp_path / "probe")], input="int main(void){return 0;}", text=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the C compiler cannot link -fsanitize=address,undefined,float-cast-overflow")
    subprocess.run(["make", "-C", os.path.join(REPO, "tests", "native"),
                    "../../oracle/_build/san/voxel_inputs_driver"], check=True, capture_output=True)
    exe = os.path.join(REPO, "oracle", "_build", "san", "voxel_inputs_driver")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")

    def run(mesh, kd):
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        with open(fin, "wb") as f:
            f.write(struct.pack("<4I", mesh.n, mesh.verts.shape[0], mesh.idx.size // 3, kd.shape[0]))
            f.write(np.array([*mesh.g0, mesh.E], F).tobytes())
            for a in (mesh.verts, mesh.idx, mesh.mat, kd):
                f.write(np.ascontiguousarray(a).tobytes())
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120, env=env)
        bad = [m for m in ("AddressSanitizer", "runtime error", "LeakSanitizer") if m in p.stderr]
        assert p.returncode == 0 and not bad and p.stdout.startswith("ok"), (p.returncode, p.stderr[-3000:])
        raw = open(fout, "rb").read()
        nv = mesh.n ** 3
        rc = struct.unpack("<i", raw[:4])[0]
        sums = np.frombuffer(raw, np.int64, nv * 6, 4).reshape(nv, 6)
        counts = np.frombuffer(raw, np.uint32, nv, 4 + nv * 48)
        vox = np.frombuffer(raw, np.uint32, nv * 8, 4 + nv * 52)
        return rc, sums, counts, vox

    for n, pl in GRIDS:
        mesh = VI.build(VI.FAMILIES, n, pl)
        rc, sums, counts, vox = run(mesh, mesh.kd)
        ref = _vox(oracle_mod, mesh)
        assert rc == 0 and np.array_equal(sums, ref[0]) and np.array_equal(counts, ref[1])
        ao, nm = oracle_mod.resolve(n, *ref)
        assert np.array_equal(vox, np.concatenate([ao.ravel(), nm.ravel()]).view(np.uint32))
    mesh = VI.build(("materials",), 8)
    for comp, val in BAD_KD:
        kd = mesh.kd.copy()
        kd[3, comp] = val
        assert run(mesh, kd)[0] == -2
