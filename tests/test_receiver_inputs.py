"""The "shadow-walk receiver rule" of include/vct_spec.h on the CPU: the rule against the start
test it replaces over every q an int holds, the hostile-receiver catalogue
(tests/receiver_inputs.py) through every reference -- the oracle's composite, the CPU backend's
vct_composite_device, tests/lights_ref.py and tests/shadow_ref.py -- against the V written down
by hand, on the field with the occupied slabs and on the open one, the length of every
reference walk, and the oracle under -fsanitize=address,undefined,float-cast-overflow on the
catalogue (a stand-alone driver run as a child process).  Every comparison is bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

import light_inputs as LI
import lights_ref
import receiver_inputs as RI
import shadow_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
N = RI.N_GRID
FIELDS = ("slabs", "open")


@pytest.fixture(scope="module")
def cat():
    return RI.catalogue()


@pytest.fixture(scope="module")
def rig(oracle_mod, cat):
    """field name -> (field, albedo_occ, normal, occ, composite frame, planes frame), once."""
    out = {}
    for name in FIELDS:
        f = RI.field(name)
        ao, nm = LI.voxels(oracle_mod, f)
        RI.check_field(name, ao)
        out[name] = (f, ao, nm, ao[..., 3] != 0, RI.build(f, ao, nm, cat), RI.build(f, ao, nm, cat, composite=False))
    return out


# ---------------------------------------------------------------------------
# the rule and the test it replaces
# ---------------------------------------------------------------------------
def _chain(start, toward, steps):
    out, v = [], F(start)
    for _ in range(steps):
        out.append(v)
        v = np.nextafter(v, F(toward))
    return out


def test_rule_equals_the_old_start_test():
    """0 <= q_a < n in float32 against floor(q_a) in [0, n) on the converted cell, for every q an
    int holds: 64 neighbours on either side of 0 (both zeros, the denormals), of n, of 1 and
    n - 1, the ends of the int range (-2^31 upwards, prev(2^31) downwards), the smallest normals,
    and 6000 random finite q, for n = 2, 16 and 1024.  So no defined result changes."""
    two31 = F(2.0 ** 31)
    rng = np.random.default_rng(11)
    for n in (2, 16, 1024):
        qs = [F(0.0), F(-0.0)]
        for c in (0.0, -0.0, 1.0, n - 1.0, float(n), n + 1.0, -1.0, 2.0 ** -126, -(2.0 ** -126), 0.5, n - 0.5):
            qs += _chain(c, np.inf, 64) + _chain(c, -np.inf, 64)
        qs += _chain(-two31, 0.0, 64) + _chain(np.nextafter(two31, F(0)), 0.0, 64)
        qs += [F(v) for v in range(-3, n + 4)]
        b = rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(F)    # any bit pattern ...
        b = b[np.isfinite(b) & (b >= -two31) & (b < two31)]                                  # ... an int holds
        qs = np.concatenate([np.array(qs, F), b, rng.uniform(-2.0, n + 2.0, 2000).astype(F)])
        assert np.isfinite(qs).all() and qs.min() == -two31 and qs.max() == np.nextafter(two31, F(0))
        assert len(qs) > 6000
        for a in range(3):                                   # one axis at a time, the others inside
            q = np.full((len(qs), 3), 0.5, F)
            q[:, a] = qs
            new, old = lights_ref.walk_starts(q, n), RI.old_start_test(q, n)
            assert np.array_equal(new, old), (n, a, qs[new != old][:8])
            assert new.any() and not new.all()
        q = qs[rng.integers(0, len(qs), (20000, 3))]         # and all three at once
        assert np.array_equal(lights_ref.walk_starts(q, n), RI.old_start_test(q, n))
    # what the old test left open: the rule says "outside" for each
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 31, -(2.0 ** 31) - 256.0, 3.4e38], F)
    q = np.full((len(bad), 3), 0.5, F)
    q[:, 1] = bad
    assert not lights_ref.walk_starts(q, 16).any()
    assert lights_ref.walk_starts(np.array([[-0.0, 0.0, np.nextafter(F(16), F(0))]], F), 16).all()
    assert not lights_ref.walk_starts(np.array([[-1e-45, 1.0, 1.0]], F), 16).any()        # a denormal is not flushed


def test_catalogue(cat, rig):
    """What the catalogue promises: the family sizes, the exact q of every edge entry (bit for
    bit, -0.0 included), NaN where the name says NaN, and frames of at most 64 x 48."""
    sizes = {f: sum(e.family == f for e in cat) for f in RI.FAMILIES}
    assert sizes == {"nan_axis": 112, "big": 240, "edge": 114, "w": 32}
    for e in cat:
        q = RI.origin(e.P[None], e.N[None])[0]
        if e.q is not None:
            assert RI.bits(q[e.q[0]]) == RI.bits(e.q[1]), (e.name, q)
            others = [a for a in range(3) if a != e.q[0]]
            assert lights_ref.walk_starts(np.array([[0.5, q[others[0]], q[others[1]]]], F), N).all(), e.name
        if e.family == "nan_axis":
            tag = e.name.split("_")[1]
            assert [bool(np.isnan(q[a])) for a in range(3)] == [c in tag for c in "xyz"], (e.name, q)
        if e.family in ("nan_axis", "big") or e.expect == "one":
            assert not lights_ref.walk_starts(q[None], N)[0], e.name
        if e.expect == "floor":
            assert lights_ref.walk_starts(q[None], N)[0], e.name
    assert sum(e.expect == "floor" for e in cat) >= 30
    for name in FIELDS:
        fr = rig[name][4]
        assert fr.pos.shape[1] == 64 and fr.pos.shape[0] <= 48 and (fr.entry >= 0).sum() == sum(not e.planes_only for e in cat)
        assert np.isfinite(fr.alb).all() and np.isfinite(fr.D).all() and np.isfinite(fr.S).all()
        assert (rig[name][5].entry >= 0).sum() == len(cat)
    assert len(RI.directions()) == 20


def test_slabs_catch_a_missing_guard(cat, rig):
    """Why the GPU tests run the slabs field and only that one.  Under a model of the device's
    arithmetic without the rule (NaN converts to cell 0), every walked nan_axis entry on the slabs
    ends in its first cell with V = 0 -- a wrong value, which the comparisons catch -- whatever the
    light; on the open field the same arithmetic does not end within 10 000 cells for P.y = NaN,
    N = +y under the light straight up, which is why that field stays with the CPU references."""
    occ_s, occ_o = rig["slabs"][3], rig["open"][3]
    wrong = 0
    for e in RI.directions():
        l = LI.normalised(e.d)
        for ent in cat:
            if ent.family != "nan_axis" or ent.planes_only or not RI.ndl_of(ent.N, e.d) > 0:
                continue
            q = RI.origin(ent.P[None], ent.N[None])[0]
            V, cells = RI.unguarded_device_walk(occ_s, q, l, 3 * N)
            assert (V, cells) == (0.0, 1), (ent.name, e.name, V, cells)
            wrong += 1
    assert wrong >= 300
    ent = next(x for x in cat if x.name == "nan_y_P_n2")
    assert np.array_equal(ent.N, np.array([0, 1, 0], F))
    V, cells = RI.unguarded_device_walk(occ_o, RI.origin(ent.P[None], ent.N[None])[0], np.array([0, 1, 0], F), 10000)
    assert V is None and cells == 10000


# ---------------------------------------------------------------------------
# every reference against the hand-written V
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_lib(oracle_mod):
    import ctypes as C
    from vct import _lib
    return _lib.bind(C.CDLL(oracle_mod.CPU_BACKEND))


@pytest.mark.parametrize("name", FIELDS)
def test_composites_give_the_hand_written_v(oracle_mod, cpu_lib, cat, rig, name):
    """Every entry x every directional light: the oracle's composite, the CPU backend's
    vct_composite_device (ctypes) and lights_ref.composite equal the numpy restatement around the
    hand-written V bit for bit: 1 for the NaN and out-of-range entries, what floor gives for
    the edge entries."""
    import vct
    from vct import Context
    f, ao, nm, occ, fr, _ = rig[name]
    h, w = fr.entry.shape
    ctx = Context(f.n, f.g0, f.E, lib=cpu_lib)
    ctx.voxelize(f.verts, f.idx, f.mat, f.kd)
    ptr = lambda a: int(a.ctypes.data)
    lin, rgba = np.empty((h, w, 4), F), np.empty((h, w), np.uint32)
    hostile = fr.entry >= 0
    seen_walked = np.zeros((h, w), bool)
    blocked = 0
    for e in RI.directions():
        V = RI.expected_v(fr, cat, occ, e.d)
        want = RI.composite_expect(fr, e.d, RI.COLOUR, V)
        assert np.isfinite(want).all(), e.name
        o_lin, o_rgba = oracle_mod.composite(f.n, f.g0, f.E, ao, fr.pos, fr.nrm, fr.alb, fr.D, fr.S, e.d, RI.COLOUR)
        d = (RI.bits(o_lin) != RI.bits(want)).any(-1)
        assert not d.any(), (name, e.name, "oracle", RI.describe(fr, d))
        lin.fill(7.0)
        ctx.composite_device(ptr(fr.pos), ptr(fr.nrm), ptr(fr.alb), ptr(fr.D), ptr(fr.S), w, h, e.d, RI.COLOUR,
                             out_linear4=ptr(lin), out_rgba8=ptr(rgba))
        d = (RI.bits(lin) != RI.bits(want)).any(-1)
        assert not d.any() and np.array_equal(rgba, o_rgba), (name, e.name, "cpu backend", RI.describe(fr, d))
        l_lin = lights_ref.composite(f.n, f.g0, f.E, ao, fr.pos, fr.nrm, fr.alb, fr.D, fr.S,
                                     [vct.directional_light([float(v) for v in e.d], RI.COLOUR)])
        d = (RI.bits(l_lin) != RI.bits(want)).any(-1)
        assert not d.any(), (name, e.name, "lights_ref", RI.describe(fr, d))
        seen_walked |= ~np.isnan(V)
        blocked += int((V[hostile] == 0).sum())
        one = np.array([i >= 0 and cat[i].expect == "one" for i in fr.entry.ravel()]).reshape(h, w)
        assert (V[one & ~np.isnan(V)] == 1).all() and (one & ~np.isnan(V)).sum() >= 50, e.name
    bg = np.array([i >= 0 and cat[i].expect == "background" for i in fr.entry.ravel()]).reshape(h, w)
    assert seen_walked[hostile & ~bg].all(), "every entry is walked under some light"
    assert not seen_walked[bg].any() and bg.sum() == 8
    # on the slabs the edge entries in cell 0 are blocked in their first cell; on the open field they walk on
    assert (blocked > 20) if name == "slabs" else True
    ctx.close()


@pytest.fixture(scope="module")
def alpha(rig):
    """The alpha pyramid of each field (level 0 alpha = occupancy; the colours do not enter it)."""
    out = {}
    for name in FIELDS:
        ao = rig[name][1]
        l0 = np.zeros_like(ao)
        l0[..., 3] = (ao[..., 3] != 0).astype(F)
        out[name] = shadow_ref.alpha_pyramid(N, l0, True)
    return out


@pytest.mark.parametrize("name", FIELDS)
def test_shadow_ref_gives_the_hand_written_v(cat, rig, alpha, name):
    """shadow_ref on every entry (the (+inf) + (-inf) family included) and the whole light
    list: a hard directional plane is the hand-written V (+0 where the light is skipped); the
    point and the spot light skip every NaN receiver by r2 > 0; a soft light gives every NaN or
    far-out receiver (the nan_axis, big and w families) V = 1 with no step, so the hard and the soft V agree."""
    f, ao, nm, occ, _, fr = rig[name]
    lights = RI.light_list()
    dirs = RI.directions()
    hard = shadow_ref.shadow(N, f.g0, f.E, ao, alpha[name], True, fr.pos, fr.nrm, lights, [0.0] * len(lights))
    assert hard["steps"] == 0
    for j, e in enumerate(dirs):
        V = RI.expected_v(fr, cat, occ, e.d)
        want = np.where(np.isnan(V), F(0), V).astype(F)
        d = RI.bits(hard["vis"][j]) != RI.bits(want)
        assert not d.any(), (name, e.name, RI.describe(fr, d))
    q = RI.origin(fr.pos, fr.nrm).reshape(-1, 3)
    valid = (fr.pos[..., 3] != 0).ravel()
    nanq = np.isnan(q).any(-1) & valid
    assert nanq.sum() == 112 + 24                                  # nan_axis, and the valid w entries
    for j in (len(dirs), len(dirs) + 1):
        L = lights_ref.prepare(lights[j], N, f.g0, f.E)
        cls = lights_ref.evaluate(L, q[valid], fr.nrm.reshape(-1, 4)[valid, :3])[4]
        assert cls["zero"][nanq[valid]].all() and cls["walk"].sum() > 20, j
        assert not hard["vis"][j].ravel()[nanq].any()
    # the hostile pixels alone, soft: nothing marches from a NaN or out-of-range q
    # (an edge entry just outside the grid, q_a = n or -1e-45, marches back into it: not part of this)
    one = np.array([i >= 0 and cat[i].expect == "one" and cat[i].family != "edge" for i in fr.entry.ravel()])
    pos, nrm = fr.pos.reshape(-1, 4)[one][None], fr.nrm.reshape(-1, 4)[one][None]
    soft = shadow_ref.shadow(N, f.g0, f.E, ao, alpha[name], True, pos, nrm, lights, [0.1] * len(lights))
    hard1 = shadow_ref.shadow(N, f.g0, f.E, ao, alpha[name], True, pos, nrm, lights, [0.0] * len(lights))
    assert soft["steps"] == 0
    assert np.array_equal(RI.bits(soft["vis"]), RI.bits(hard1["vis"]))
    assert set(np.unique(soft["vis"]).tolist()) == {0.0, 1.0} and (soft["vis"] == 1).sum() > 1000
    walked = sum(p["px"].size for p in soft["pairs"])
    assert walked == int((soft["vis"] == 1).sum())               # V = 1 for every pair not skipped


@pytest.mark.parametrize("name", FIELDS)
def test_every_reference_walk_ends_within_3n_cells(cat, rig, name):
    """The cells lights_ref.walk tests, per receiver, for every entry and every light of the list
    (point and spot included): at most 3 n (a walk crosses at most n cells per axis), and none
    from a q that fails the rule."""
    f, ao, nm, occ, _, fr = rig[name]
    valid = (fr.pos[..., 3] != 0).ravel()
    q = RI.origin(fr.pos, fr.nrm).reshape(-1, 3)[valid]
    Nn = fr.nrm.reshape(-1, 4)[valid, :3]
    longest = 0
    for light in RI.light_list():
        L = lights_ref.prepare(light, N, f.g0, f.E)
        l, fac, ndl, t_lim, cls = lights_ref.evaluate(L, q, Nn)
        k = np.flatnonzero(cls["walk"])
        cells = np.zeros(k.size, np.int64)
        V, end = lights_ref.walk(occ, q[k], l[k], t_lim[k], cells)
        assert cells.max() <= 3 * N
        out = ~lights_ref.walk_starts(q[k], N)
        assert out.any() and not cells[out].any() and (V[out] == 1).all()
        longest = max(longest, int(cells.max()))
    print(f"{name}: longest reference walk {longest} cells")
    assert longest >= (N // 2 if name == "open" else 2)


# ---------------------------------------------------------------------------
# the oracle under sanitizers on the catalogue
# ---------------------------------------------------------------------------
def test_oracle_composite_under_sanitizers(oracle_mod, cat, rig, tmp_path):
    """oracle/vct_oracle.c built with -fsanitize=address,undefined,float-cast-overflow runs
    vo_composite over the catalogue on both fields under every direction, in a child process: no
    report (no float -> int conversion of a NaN, an infinity or a value past the int range), every
    walk ends, and the same bits as the oracle library."""
    probe = subprocess.run(["gcc", "-fsanitize=address,undefined,float-cast-overflow", "-x", "c", "-", "-o",
                            str(tmp_path / "probe")], input="int main(void){return 0;}", text=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the C compiler cannot link -fsanitize=address,undefined,float-cast-overflow")
    subprocess.run(["make", "-C", os.path.join(REPO, "tests", "native"),
                    "../../oracle/_build/san/receiver_inputs_driver"], check=True, capture_output=True)
    exe = os.path.join(REPO, "oracle", "_build", "san", "receiver_inputs_driver")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    dirs = RI.directions()
    # one frame for both fields: the slabs frame (its clean pixels are ordinary receivers on the open field too)
    fr = rig["slabs"][4]
    h, w = fr.entry.shape
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<5I", N, len(FIELDS), len(dirs), w, h))
        fh.write(np.array([*RI.G0, RI.E], F).tobytes())
        for a in [rig[name][1] for name in FIELDS] + [np.array([e.d for e in dirs], F),
                                                      np.array([RI.COLOUR] * len(dirs), F), fr.pos, fr.nrm, fr.alb, fr.D, fr.S]:
            fh.write(np.ascontiguousarray(a, F).tobytes())
    p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120, env=env)
    bad = [m for m in ("AddressSanitizer", "runtime error", "LeakSanitizer") if m in p.stderr]
    assert p.returncode == 0 and not bad and p.stdout.startswith("ok"), (p.returncode, p.stderr[-3000:])
    px = w * h
    raw = np.fromfile(fout, np.uint32).reshape(len(FIELDS), len(dirs), px * 5)
    for k, name in enumerate(FIELDS):
        for i, e in enumerate(dirs):
            lin, rgba = oracle_mod.composite(N, RI.G0, RI.E, rig[name][1], fr.pos, fr.nrm, fr.alb, fr.D, fr.S, e.d, RI.COLOUR)
            assert np.array_equal(raw[k, i, :px * 4], RI.bits(lin).ravel()), (name, e.name)
            assert np.array_equal(raw[k, i, px * 4:], rgba.ravel()), (name, e.name)
