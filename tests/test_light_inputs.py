"""The hostile-light catalogue (tests/light_inputs.py) and its references, on the CPU: what the
catalogue promises by construction (list sizes, integer-q shares, exit lengths), the Python
restatements of the A.3 shadow walk against the C oracle over every legal entry (bit-exact:
the expected values of the GPU tests rest on independent restatements), what the K2 input
rule of include/vct_spec.h changed against the walk as it was, the rule's errors on the CPU
backend, and the oracle under -fsanitize=address,undefined,float-cast-overflow on the
catalogue (a stand-alone driver run as a child process)."""
import os
import subprocess

import numpy as np
import pytest

import light_inputs as LI
import lights_ref
import spec_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EINVAL = 1
SIZES = {"axis": 36, "planar": 36, "ties": 78, "tiny": 180, "edge": 30, "nonfinite": 27}


@pytest.fixture(scope="module")
def vox(oracle_mod):
    """field name -> (field, albedo_occ, normal) through the oracle's K1, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            f = LI.field(name)
            cache[name] = (f,) + LI.voxels(oracle_mod, f)
        return cache[name]
    return get


def _lit(N, d):
    l = LI.normalised(d)
    return ((N[:, 0] * l[0] + N[:, 1] * l[1]) + N[:, 2] * l[2]) > 0


def test_catalogue_entries():
    dirs = LI.directions()
    sizes = {f: sum(e.family == f for e in dirs) for f in LI.DIR_FAMILIES}
    print("directions per family:", sizes, "legal", len(LI.legal_directions()), "illegal", len(LI.illegal_directions()))
    assert sizes == SIZES
    assert all(LI.direction_status(e.d) == EINVAL for e in dirs if e.family == "nonfinite")
    assert all(LI.direction_status(e.d) == 0 for e in dirs if e.family in ("axis", "planar", "ties", "tiny"))
    # the edge family on both sides of the rule, by the rule: squared length 0 and +inf refused,
    # a denormal and the largest finite squared length accepted
    st = {e.name: LI.direction_status(e.d) for e in dirs if e.family == "edge"}
    assert st["edge_sq_min_normal"] == st["edge_sq_denormal"] == st["edge_sq_denormal3"] == st["edge_sq_max_finite"] == 0
    assert st["edge_sq_zero"] == st["edge_sq_zero_denormals"] == st["edge_zero"] == st["edge_sq_inf"] == EINVAL
    assert st["edge_sq_sum_inf"] == st["edge_max_float"] == EINVAL
    with np.errstate(all="ignore"):
        sq = lambda d: (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        by = {e.name: sq(e.d) for e in dirs}
    tiny32 = np.finfo(F).tiny
    assert by["edge_sq_min_normal"] == tiny32 and 0 < by["edge_sq_denormal"] < tiny32 and by["edge_sq_zero"] == 0
    assert np.isfinite(by["edge_sq_max_finite"]) and by["edge_sq_max_finite"] > 3.4e38 and np.isinf(by["edge_sq_inf"])
    # td of the tiny family: finite down to 2^-126, +inf for the denormals
    with np.errstate(all="ignore"):
        for e in LI.legal_directions(("tiny",), raw_only=True):
            td = F(1.0) / np.abs(LI.normalised(e.d))
            assert np.isinf(td).any() == ("1e-40" in e.name or "1e-45" in e.name), e.name
    assert len(LI.sample_directions()) >= 12
    assert [LI.colour_status(c.c) for c in LI.COLOURS] == [0, 0, 1, 1, 0, 1, 1, 1, 1, 1]
    assert float(LI.COLOR_LIMIT) == 2.0 ** 127 / (32768.0 * 2.0 * 64.0)


def test_field_conditions(vox):
    """What the field names promise, through the oracle."""
    up = np.array([0.0, 0.0, 1.0], F)
    want_occ = {"counts64_occ4095": 4095, "counts64_occ4096": 4096, "counts64_occ4097": 4097, "counts16_lit255": 255,
                "counts16_lit256": 256, "counts16_lit257": 257, "counts8_one": 1, "counts8_full": 512, "counts8_none": 0}
    for name, cnt in want_occ.items():
        f, ao, nm = vox(name)
        (z, y, x), q, N, A = LI.receivers(ao, nm)
        assert len(x) == cnt, (name, len(x))
        if "lit" in name:
            assert _lit(N, up).sum() == cnt, name
    # integer q on the axis of the denormal component
    for name in LI.FIELD_NAMES:
        if not name.startswith("integer_q"):
            continue
        f, ao, nm = vox(name)
        (z, y, x), q, N, A = LI.receivers(ao, nm)
        a, d = LI.integer_q_light(name)
        both = _lit(N, d) & (q[:, a] == np.floor(q[:, a]))
        print(f"{name}: {len(x)} occupied, {int(both.sum())} lit with an integer q on axis {a}")
        assert both.sum() >= 100 and len(np.unique(N, axis=0)) == 1
        assert abs(abs(float(N[0, a])) - 0.49999973) < 1e-8
    # faces: the flush box's receivers start outside the grid, the inner box's inside
    f, ao, nm = vox("faces8_flush")
    (z, y, x), q, N, A = LI.receivers(ao, nm)
    assert len(x) == 8 ** 3 - 6 ** 3 and np.all(np.any((np.floor(q) < 0) | (np.floor(q) >= 8), axis=1))
    assert (A < 0).any() and (A > 0).any()
    f, ao, nm = vox("faces8_inside")
    (z, y, x), q, N, A = LI.receivers(ao, nm)
    assert len(x) == 6 ** 3 - 4 ** 3 and np.all((np.floor(q) >= 0) & (np.floor(q) < 8))
    # sizes
    for n in (4, 8, 16, 64, 128):
        f, ao, nm = vox(f"sizes{n}")
        assert f.n == n and (ao[..., 3] != 0).sum() > n * n // 2


def test_exits(vox):
    """The exits field: every row's walk tests the cells its name says, an occluder in the
    wrapped cell does not count, and over the axis, planar and ties directions the walks that
    leave the grid do so after every number of cells from 1 to 40."""
    f, ao, nm = vox("exits32")
    occ = ao[..., 3] != 0
    (z, y, x), q, N, A = LI.receivers(ao, nm)
    at = {(int(a), int(b), int(c)): i for i, (a, b, c) in enumerate(zip(x, y, z))}
    for axis in (0, 1):
        l = np.zeros(3, F)
        l[axis] = 1.0
        for k, a, b, kind in LI.exit_rows(axis):
            i = at[LI.exit_cell(axis, 31 - k, a, b)]
            V, cells, left = LI.walk_count(occ, q[i:i + 1], l)
            if kind in (None, "wrap") or k == 1:
                want = (1.0, k)
            else:
                want = (0.0, 1 if kind == "first" else k)
            assert (float(V[0]), int(cells[0])) == want, (axis, k, kind)
            if kind == "wrap":
                assert occ[LI.exit_cell(axis, 0, a + 1, b)[::-1]]
    seen = set()
    for e in LI.legal_directions(("axis", "planar", "ties"), raw_only=True):
        lit = _lit(N, e.d)
        V, cells, left = LI.walk_count(occ, q[lit], LI.normalised(e.d))
        seen |= set(cells[left].tolist())
    assert set(range(1, 41)) <= seen, sorted(set(range(1, 41)) - seen)


def _oracle_all(O, f, ao, nm, dirs, colour=(1.0, 1.0, 1.0)):
    return np.stack([O.inject(f.n, ao, nm, e.d, colour) for e in dirs])


@pytest.mark.parametrize("name", LI.SMALL_FIELDS + ["sizes64"])
def test_restatement_equals_oracle(oracle_mod, vox, name):
    """light_inputs.walk_count (the K2 input rule restated in numpy, every receiver and direction
    in lockstep) against vo_inject over every legal direction, the whole of level 0, bit for bit."""
    f, ao, nm = vox(name)
    dirs = LI.legal_directions() if f.n <= 32 else LI.sample_directions()
    chunk = 64 if f.n <= 16 else 16
    lit = 0
    for i in range(0, len(dirs), chunk):
        part = dirs[i:i + chunk]
        got = LI.inject_batch(ao, nm, [e.d for e in part], (1.0, 0.5, 0.25))
        want = _oracle_all(oracle_mod, f, ao, nm, part, (1.0, 0.5, 0.25))
        same = (LI.bits(got) == LI.bits(want)).reshape(len(part), -1).all(axis=1)
        assert same.all(), (name, [e.name for e, s in zip(part, same) if not s][:5])
        lit += int((want[..., :3] != 0).any(-1).sum())
    assert lit > 0 or name == "counts8_none"


@pytest.mark.parametrize("name", ["integer_q16_x+", "integer_q16_y-", "faces8_inside", "sizes8"])
def test_lights_ref_and_spec_ref_equal_oracle(oracle_mod, vox, name):
    """The two older restatements, which the rule changed: tests/lights_ref.py (a one-light list
    is vct_inject_directional bit for bit) over every raw legal direction, tests/spec_ref.py (pure
    Python, slow) over the td = +inf entries."""
    import vct
    f, ao, nm = vox(name)
    for e in LI.legal_directions(raw_only=True):
        want = oracle_mod.inject(f.n, ao, nm, e.d, (1.0, 0.5, 0.25))
        got = lights_ref.inject(f.n, f.g0, f.E, ao, nm, [vct.directional_light(e.d, (1.0, 0.5, 0.25))])
        # a list starts from acc = +0: a contribution of -0 (negative albedo, V = 0) becomes +0
        assert np.array_equal(LI.bits(got), LI.bits(F(0) + want)), (name, e.name)
        if e.family == "tiny" and "1e-4" in e.name and f.n <= 16 and e.name.endswith("pos"):
            assert np.array_equal(LI.bits(spec_ref.inject(f.n, ao, nm, e.d, (1.0, 0.5, 0.25))), LI.bits(want)), e.name


def test_what_the_rule_changed(oracle_mod, vox):
    """The walk as it was (a NaN t makes every comparison false: the walk steps the NaN axis
    on every iteration) against the K2 input rule, which is what the kernels always did: the lit
    voxels of the integer-q quads whose level 0 differs, and nothing differs where no td is
    +inf."""
    changed = {}
    for name in ("integer_q16_x+", "integer_q16_y+", "integer_q32_x+", "integer_q32_y+"):
        f, ao, nm = vox(name)
        a, d = LI.integer_q_light(name)
        new = LI.inject_batch(ao, nm, [d])[0]
        old = LI.inject_batch(ao, nm, [d], nan_rule="parent")[0]
        assert np.array_equal(LI.bits(new), LI.bits(oracle_mod.inject(f.n, ao, nm, d)))
        changed[name] = int((LI.bits(new) != LI.bits(old)).any(-1).sum())
    print("voxels whose level 0 the rule changed:", changed)
    assert changed["integer_q16_x+"] >= 100 and changed["integer_q32_x+"] >= 1000
    f, ao, nm = vox("integer_q16_x+")
    plain = [e.d for e in LI.legal_directions(("axis", "planar", "ties"), raw_only=True)]
    plain += [e.d for e in LI.legal_directions(("tiny",), raw_only=True) if "1e-4" not in e.name]
    assert np.array_equal(LI.bits(LI.inject_batch(ao, nm, plain)), LI.bits(LI.inject_batch(ao, nm, plain, nan_rule="parent")))


def test_level0_stays_finite_at_the_limits():
    """The derivation of VCT_COLOR_LIMIT: the largest legal albedo, a unit normal facing the
    light, VCT_MAX_LIGHTS lights of the limit colour: the sum is finite (2^126 to rounding)."""
    import vct
    n = 4
    ao, nm = np.zeros((n, n, n, 4), F), np.zeros((n, n, n, 4), F)
    ao[1, 2, 3] = (np.nextafter(F(32768), F(0)),) * 3 + (1.0,)
    nm[1, 2, 3, :3] = (0.0, 1.0, 0.0)
    lights = [vct.directional_light((0.0, 1.0, 0.0), (float(LI.COLOR_LIMIT),) * 3)] * 64
    r0 = lights_ref.inject(n, (0.0, 0.0, 0.0), float(n), ao, nm, lights)
    assert np.isfinite(r0).all() and 2.0 ** 125 < r0[1, 2, 3, 0] <= 2.0 ** 126


def test_light_lists_reference(oracle_mod, vox):
    """The light-list entries do what their names say, in tests/lights_ref.py."""
    f, ao, nm = vox("lists16_exact")
    assert f.g0 == (0.0, 0.0, 0.0) and f.E == 16.0
    stats = {}
    for e in LI.light_lists():
        st = []
        r0 = lights_ref.inject(f.n, f.g0, f.E, ao, nm, e.lights, st)
        assert np.isfinite(r0).all(), e.name
        stats[e.name] = st
    walked = lambda name: [s["walked"] for s in stats[name]]
    assert walked("far_r2_finite")[0] > 0                                   # r2 ~ 6e36: finite, lit
    assert walked("far_r2_overflow") == [0, 0] and walked("far_pl_overflow") == [0, 0]
    assert walked("range_tiny") == [0] and stats["range_tiny"][0]["culled"] > 100
    assert walked("range_denormal_rr") == [0]
    assert walked("range_huge")[0] > 100 and stats["range_huge"][0]["culled"] == 0
    assert walked("spot_ulp_half")[0] > 0 and stats["spot_ulp_half"][0]["culled"] > 0
    assert all(w > 0 for w in walked("inside_occupied") + walked("on_faces") + walked("outside"))
    assert all(s["reached"] > 0 for s in stats["own_cell"]) and stats["own_cell"][1]["zero"] == 1
    assert all(s["zero_l"] > 0 for s in stats["shared_coords"])
    # 0 * inf in the spot term: receivers exactly at cd = cos_outer = 0 with inv_span = +inf
    L = lights_ref.prepare(LI.light_lists()[7].lights[0], f.n, f.g0, f.E)
    assert LI.light_lists()[7].name == "spot_ulp_zero" and np.isinf(L["inv_span"])
    (z, y, x), q, N, A = lights_ref.receivers(ao, nm)
    l, fac, ndl, t_lim, cls = lights_ref.evaluate(L, q, N)
    with np.errstate(all="ignore"):
        cd = lights_ref.dot3(l[:, 0], l[:, 1], l[:, 2], *L["a"])
    # (the two specks at y = 12 that face the light)
    assert ((cd == 0) & (ndl > 0)).sum() == 2 and not fac[(cd == 0)].any() and (fac > 0).sum() > 10


COLOUR = (1.0, 0.5, 0.25)


def test_filler_formula(oracle_mod, vox):
    """The closed form (+0 + filler) + oracle, which tests/test_light_inputs_gpu.py expects of
    the 34-light lists (filler: the oracle's level 0 of the fillers' one directional light;
    oracle: that of the light under test), equals lights_ref.inject of the same list."""
    import vct
    f, ao, nm = vox("integer_q16_x+")
    fill = oracle_mod.inject(f.n, ao, nm, LI.FILLER_DIR, LI.FILLER_COLOUR)
    for e in LI.legal_directions(("tiny",), raw_only=True)[::7]:
        one = oracle_mod.inject(f.n, ao, nm, e.d, COLOUR)
        want = (F(0) + fill) + one
        want[..., 3] = one[..., 3]
        ref = lights_ref.inject(f.n, f.g0, f.E, ao, nm, LI.filler_lights() + [vct.directional_light(e.d, COLOUR)])
        assert np.array_equal(LI.bits(ref), LI.bits(want)), e.name


# ---------------------------------------------------------------------------
# the rule's errors on the CPU backend
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_lib(oracle_mod):
    import ctypes as C
    from vct import _lib
    return _lib.bind(C.CDLL(oracle_mod.CPU_BACKEND))


def test_illegal_lights_are_refused(oracle_mod, cpu_lib, vox):
    """Every illegal direction and colour: VCT_EINVAL from vct_inject_directional and
    vct_composite_device of the CPU backend, level 0 and the outputs as they were; every legal
    colour and edge direction is accepted and equals the oracle."""
    from vct import Context, VctError
    f, ao, nm = vox("sizes8")
    ctx = Context(f.n, f.g0, f.E, lib=cpu_lib)
    ctx.voxelize(f.verts, f.idx, f.mat, f.kd)
    clean = (0.3, 0.9, 0.2)
    ctx.inject_directional(clean, (1.0, 0.5, 0.25))
    before = ctx.download_level(0)
    assert np.array_equal(LI.bits(before), LI.bits(oracle_mod.inject(f.n, ao, nm, clean, (1.0, 0.5, 0.25))))
    pos, nrm, alb = LI.gbuffer_of(f, ao, nm)
    h, w = pos.shape[:2]
    D, S = np.full((h, w, 4), 0.25, F), np.full((h, w, 4), 0.125, F)
    lin = np.full((h, w, 4), 7.0, F)
    ptr = lambda a: int(a.ctypes.data)

    def composite(d, c):
        ctx.composite_device(ptr(pos), ptr(nrm), ptr(alb), ptr(D), ptr(S), w, h, d, c, out_linear4=ptr(lin))

    bad = [(e.name, e.d, (1.0, 1.0, 1.0)) for e in LI.illegal_directions()]
    bad += [(c.name, clean, c.c) for c in LI.COLOURS if LI.colour_status(c.c) != 0]
    assert len(bad) >= 45 + 6
    for name, d, c in bad:
        for call in (lambda: ctx.inject_directional(d, c), lambda: composite(d, c)):
            with pytest.raises(VctError) as ei:
                call()
            assert ei.value.status == EINVAL, name
        assert np.array_equal(LI.bits(ctx.download_level(0)), LI.bits(before)), name
        assert (lin == 7.0).all(), name
    for c in LI.COLOURS:
        if LI.colour_status(c.c) == 0:
            ctx.inject_directional(clean, c.c)
            got = ctx.download_level(0)
            assert np.isfinite(got).all(), c.name
            assert np.array_equal(LI.bits(got), LI.bits(oracle_mod.inject(f.n, ao, nm, clean, c.c))), c.name
            composite(clean, c.c)
            assert np.array_equal(LI.bits(lin), LI.bits(oracle_mod.composite(f.n, f.g0, f.E, ao, pos, nrm, alb, D, S,
                                                                              clean, c.c)[0])), c.name
    for e in LI.legal_directions(("edge",)):
        ctx.inject_directional(e.d)
        assert np.array_equal(LI.bits(ctx.download_level(0)), LI.bits(oracle_mod.inject(f.n, ao, nm, e.d))), e.name
    ctx.close()


# ---------------------------------------------------------------------------
# the oracle under sanitizers on the whole catalogue
# ---------------------------------------------------------------------------
def test_oracle_inject_under_sanitizers(oracle_mod, vox, tmp_path):
    """oracle/vct_oracle.c built with -fsanitize=address,undefined,float-cast-overflow runs
    vo_inject and vo_composite over every legal direction of the catalogue (the backend refuses
    the others before the oracle sees them) and every colour, legal or not, on the integer-q,
    faces and exits fields in a child process: no report, every walk ends, and the same bits
    as the oracle library.  Light lists are not part of it: the C oracle has no light-list path
    to put under a sanitizer (their reference is tests/lights_ref.py)."""
    import struct
    probe = subprocess.run(["gcc", "-fsanitize=address,undefined,float-cast-overflow", "-x", "c", "-", "-o",
                            str(tmp_path / "probe")], input="int main(void){return 0;}", text=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the C compiler cannot link -fsanitize=address,undefined,float-cast-overflow")
    subprocess.run(["make", "-C", os.path.join(REPO, "tests", "native"),
                    "../../oracle/_build/san/light_inputs_driver"], check=True, capture_output=True)
    exe = os.path.join(REPO, "oracle", "_build", "san", "light_inputs_driver")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    lights = [(e.d, (1.0, 0.5, 0.25)) for e in LI.legal_directions()] + [((0.3, 0.9, 0.2), c.c) for c in LI.COLOURS]
    dirs = np.array([l[0] for l in lights], F)
    cols = np.array([l[1] for l in lights], F)
    for name in ("integer_q16_x+", "integer_q16_z-", "integer_q16_y+_exact", "faces8_flush", "exits32", "sizes4"):
        f, ao, nm = vox(name)
        pos, nrm, alb = LI.gbuffer_of(f, ao, nm)
        h, w = pos.shape[:2]
        D, S = np.full((h, w, 4), 0.25, F), np.full((h, w, 4), 0.125, F)
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        with open(fin, "wb") as fh:
            fh.write(struct.pack("<4I", f.n, len(lights), w, h))
            fh.write(np.array([*f.g0, f.E], F).tobytes())
            for a in (ao, nm, dirs, cols, pos, nrm, alb, D, S):
                fh.write(np.ascontiguousarray(a, F).tobytes())
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120, env=env)
        bad = [m for m in ("AddressSanitizer", "runtime error", "LeakSanitizer") if m in p.stderr]
        assert p.returncode == 0 and not bad and p.stdout.startswith("ok"), (name, p.returncode, p.stderr[-3000:])
        nv, px = f.n ** 3 * 4, w * h * 4
        raw = np.fromfile(fout, np.uint32).reshape(len(lights), nv + px + w * h)
        for i in range(0, len(lights), 7):                              # every seventh against the library
            want = oracle_mod.inject(f.n, ao, nm, dirs[i], cols[i])
            assert np.array_equal(raw[i, :nv], LI.bits(want).ravel()), (name, i)
            lin, rgba = oracle_mod.composite(f.n, f.g0, f.E, ao, pos, nrm, alb, D, S, dirs[i], cols[i])
            assert np.array_equal(raw[i, nv:nv + px], LI.bits(lin).ravel()), (name, i)
            assert np.array_equal(raw[i, nv + px:], rgba.ravel()), (name, i)
