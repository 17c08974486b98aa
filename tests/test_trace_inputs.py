"""The hostile-pixel catalogue (tests/trace_inputs.py) and its reference, on the CPU:
the builder's placement conditions, the conditions on the oracle alone, spec_ref.Tracer.pixel
against the C oracle pixel by pixel over the catalogue (bit-exact: the expected values of
the GPU tests rest on two independent restatements), the oracle under
-fsanitize=address,undefined,float-cast-overflow on the catalogue frame (a stand-alone
driver run as a child process), and the step counts of the apertures that the step-table
tests of test_trace_inputs_gpu.py rely on."""
import os
import struct
import subprocess

import numpy as np
import pytest

import spec_ref
import trace_inputs as TI
from helpers import scene_arrays

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def cornell16(oracle_mod):
    """cornell at n = 16 on the oracle, the clean 64 x 48 frame and its trace (computed once)."""
    from vct import scenes
    from vct.camera import Camera
    n = 16
    s, (v, i, m, k) = scene_arrays("cornell")
    g0, E = scenes.grid_for_unit_box(n)
    grid = oracle_mod.pipeline(n, g0, E, v, i, m, k, scenes.LIGHT_DIR)
    cam = Camera()
    clean = scenes.raycast_numpy(s, cam, 64, 48)
    ref_clean = oracle_mod.trace(n, g0, E, grid["r0"], grid["pyr"], *clean, cam.position)
    return dict(n=n, g0=g0, E=E, grid=grid, clean=clean, eye=cam.position, ref_clean=ref_clean)


def test_catalogue_entries():
    cat = TI.catalogue((-1.0, -1.0, -1.0), 2.0, 16)
    names = [e.name for e in cat]
    assert len(set(names)) == len(names) == 59
    assert {e.family for e in cat} == set(TI.FAMILIES)
    # the exact-origin entries hit 0 and n exactly in the kernels' operation order
    for e in cat:
        if e.name[:3] in ("o0_", "on_"):
            P, N, A = np.array([0.1, 0.2, 0.3, 1], F), np.array([0, 1, 0, 0], F), np.zeros(4, F)
            e.apply(P, N, A)
            a = "xyz".index(e.name[3])
            assert TI.cone_origin(P, N, (-1.0, -1.0, -1.0), 2.0, 16)[a] == (0.0 if e.name[1] == "0" else 16.0)


def test_lane_mapping_is_a_bijection():
    seen = {TI.lane_of(x, y) for y in range(8) for x in range(8)}
    assert seen == set(range(64))
    for j in range(64):
        assert TI.lane_of(*TI.lane_xy(j)) == j
    assert TI.lane_xy(1) == (1, 0) and TI.lane_xy(2) == (0, 1) and TI.lane_xy(4) == (2, 0)


@pytest.mark.parametrize("families", [(f,) for f in TI.FAMILIES] + [TI.FAMILIES])
def test_frames_and_reference_conditions(oracle_mod, cornell16, families):
    """build() asserts the placement conditions; here every selected entry must also sit in a
    block of its own (family frames) and the oracle must meet the conditions that keep a
    comparison from passing vacuously."""
    c = cornell16
    fr = TI.build(c["clean"], c["g0"], c["E"], c["n"], families)
    want = [e.name for e in TI.catalogue(c["g0"], c["E"], c["n"]) if e.family in families]
    if len(families) == 1:
        assert fr.isolated == want
        assert fr.mixed_block is None
    else:
        assert fr.mixed_block is not None and len(fr.isolated) >= 30
        assert set(want) == {w[0] for w in fr.where}
    assert TI.build(c["clean"], c["g0"], c["E"], c["n"], families).pos.tobytes() == fr.pos.tobytes()
    ref = oracle_mod.trace(c["n"], c["g0"], c["E"], c["grid"]["r0"], c["grid"]["pyr"], fr.pos, fr.nrm, fr.alb,
                           c["eye"])
    TI.check_reference(ref, c["ref_clean"], fr, c["clean"])


def test_eye_frames_reference(oracle_mod, cornell16):
    c = cornell16
    eye, (y, x) = TI.eye_on_pixel(c["clean"])
    for e in (eye, TI.EYE_FAR):
        ref = oracle_mod.trace(c["n"], c["g0"], c["E"], c["grid"]["r0"], c["grid"]["pyr"], *c["clean"], e)
        assert np.isfinite(ref["diffuse"]).all() and np.isfinite(ref["spec"]).all()
        assert np.array_equal(ref["diffuse"], c["ref_clean"]["diffuse"])     # the eye moves the specular cone only
    ref = oracle_mod.trace(c["n"], c["g0"], c["E"], c["grid"]["r0"], c["grid"]["pyr"], *c["clean"], eye)
    assert not ref["spec"][y, x].any()                                        # vl = 0: a NaN reflection, no step


# ---------------------------------------------------------------------------
# B.1  spec_ref.Tracer.pixel against the C oracle over the catalogue
# ---------------------------------------------------------------------------
def _small_level0(n, seed=3):
    rng = np.random.default_rng(seed)
    occ = rng.random((n, n, n)) < 0.06
    r0 = np.zeros((n, n, n, 4), F)
    r0[occ] = rng.random((int(occ.sum()), 4)).astype(F)
    return r0


def test_spec_ref_matches_oracle_over_catalogue(oracle_mod):
    """Every catalogue entry, applied to two base pixels (normals on either side of the
    tangent basis' sign branch), and the two eye cases (over an unedited in-grid pixel and
    the entries that do not move P: vl = 0 and the 0/0 of fdiv are reached): spec_ref.Tracer.pixel equals
    oracle_mod.trace bit for bit (outputs through a uint32 view, steps equal).  n = 16,
    g0 = 0 (so pos_denorm is a true denormal offset), a random sparse level 0."""
    O = oracle_mod
    n, g0, E = 16, (0.0, 0.0, 0.0), 1.0
    r0 = _small_level0(n)
    pyr = O.build_mips(n, r0, True)
    tr = spec_ref.Tracer(n, g0, E, r0, O.pyramid_levels(n, pyr, True), aniso=True)
    cat = TI.catalogue(g0, E, n)
    bases = [(np.array([0.5, 0.4, 0.6, 1.0], F), np.array([0.36, 0.48, 0.8, 0.0], F)),
             (np.array([0.3, 0.7, 0.45, 1.0], F), np.array([0.6, 0.0, -0.8, 0.0], F))]
    eye = (0.5, 0.6, 2.5)
    px, names = [], []
    for bi, (bp, bn) in enumerate(bases):
        for e in cat if bi == 0 else [e for e in cat if e.family in ("normal", "nonfinite", "posw")]:
            P, N, A = bp.copy(), bn.copy(), np.array([0.7, 0.6, 0.5, 0.1], F)
            with np.errstate(all="ignore"):
                e.apply(P, N, A)
            px.append((P, N, A))
            names.append(e.name)
    # the eye cases run over an unedited in-grid pixel and the entries that leave P alone
    # (pos.w, normal, roughness), so the eye can equal a pixel's position bit for bit
    P0, N0, A0 = bases[0][0].copy(), bases[0][1].copy(), np.array([0.7, 0.6, 0.5, 0.1], F)
    eye_px = [len(px)] + [j for j in range(len(cat)) if cat[j].family in ("posw", "normal", "roughness")]
    px.append((P0, N0, A0))
    names.append("unedited")
    pos, nrm, alb = (np.stack([p[k] for p in px])[None] for k in range(3))
    on_px = tuple(float(v) for v in P0[:3])
    eyes = [(eye, range(len(px))), (on_px, eye_px), (TI.EYE_FAR, eye_px)]
    for e, idx in eyes:
        ref = O.trace(n, g0, E, r0, pyr, pos, nrm, alb, e)
        assert np.isfinite(ref["diffuse"]).all() and np.isfinite(ref["spec"]).all()
        for j in idx:
            d, s, st = tr.pixel(pos[0, j], nrm[0, j], alb[0, j, 3], e)
            got = np.array([d, s], F).view(np.uint32)
            want = np.stack([ref["diffuse"][0, j], ref["spec"][0, j]]).view(np.uint32)
            assert np.array_equal(got, want), (names[j], e, d, s, ref["diffuse"][0, j], ref["spec"][0, j])
            assert st == ref["steps_px"][0, j], (names[j], e, st, int(ref["steps_px"][0, j]))
        if e is on_px:
            # vl = 0 is really reached: the eye is bit-equal to these pixels' positions, their
            # reflection is NaN (no specular step, all zeros) while their diffuse cones step
            hit = [j for j in idx if np.array_equal(pos[0, j, :3].view(np.uint32), np.array(e, F).view(np.uint32))
                   and pos[0, j, 3] != 0]
            assert len(hit) >= 20 and len(px) - 1 in hit
            assert all(not ref["spec"][0, j].view(np.uint32).any() for j in hit)
            assert sum(int(ref["steps_px"][0, j]) > 0 for j in hit) >= 15
            on_steps = int(ref["steps_px"][0, len(px) - 1])
        if e is TI.EYE_FAR:
            # a zero reflection: the specular cone stays at its origin and takes steps (the
            # diffuse cones take the same steps under either eye, the NaN reflection none)
            assert ref["steps_px"][0, len(px) - 1] > on_steps
    assert ref["steps_px"].any()


def test_ieee_helpers():
    inf, nan = float("inf"), float("nan")
    assert spec_ref.f32(1e39) == inf and spec_ref.f32(-1e39) == -inf and spec_ref.f32(3.4028235e38) < inf
    assert spec_ref.fdiv(1.0, 0.0) == inf and spec_ref.fdiv(-1.0, 0.0) == -inf and spec_ref.fdiv(1.0, -0.0) == -inf
    assert spec_ref.fdiv(0.0, 0.0) != spec_ref.fdiv(0.0, 0.0) and spec_ref.fdiv(6.0, 3.0) == 2.0
    assert spec_ref.fmaxf(nan, 0.02) == 0.02 and spec_ref.fmaxf(0.02, nan) == 0.02
    assert spec_ref.fminf(nan, 1.0) == 1.0 and spec_ref.fminf(5.0, 1.0) == 1.0 and spec_ref.fmaxf(-inf, 0.02) == 0.02
    assert spec_ref.fmaf(inf, 0.0, 1.0) != spec_ref.fmaf(inf, 0.0, 1.0)          # NaN
    assert spec_ref.fmaf(inf, 1.0, 1.0) == inf and spec_ref.fmaf(0.0, 2.0, 3.0) == 3.0
    assert spec_ref.fmaf(3e38, 2.0, 0.0) == inf


# ---------------------------------------------------------------------------
# B.2  the oracle under sanitizers on the catalogue frame
# ---------------------------------------------------------------------------
def test_oracle_trace_under_sanitizers(oracle_mod, cornell16, tmp_path):
    """oracle/vct_oracle.c built with -fsanitize=address,undefined,float-cast-overflow runs
    vo_build_mips and vo_trace over the whole catalogue frame (and the two eye cases) in a
    child process: no report, and the same bits as the oracle library."""
    probe = subprocess.run(["gcc", "-fsanitize=address,undefined,float-cast-overflow", "-x", "c", "-", "-o",
                            str(tmp_path / "probe")], input="int main(void){return 0;}", text=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the C compiler cannot link -fsanitize=address,undefined,float-cast-overflow")
    subprocess.run(["make", "-C", os.path.join(REPO, "tests", "native"),
                    "../../oracle/_build/san/trace_inputs_driver"], check=True, capture_output=True)
    exe = os.path.join(REPO, "oracle", "_build", "san", "trace_inputs_driver")
    c = cornell16
    fr = TI.build(c["clean"], c["g0"], c["E"], c["n"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    h, w = fr.pos.shape[:2]
    for eye in (c["eye"], TI.eye_on_pixel(c["clean"])[0], TI.EYE_FAR):
        fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
        with open(fin, "wb") as f:
            f.write(struct.pack("<6I", c["n"], 1, 9, 1, w, h))
            f.write(np.array([*c["g0"], c["E"], *eye], F).tobytes())
            for a in (c["grid"]["r0"], fr.pos, fr.nrm, fr.alb):
                f.write(np.ascontiguousarray(a, F).tobytes())
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120, env=env)
        bad = [m for m in ("AddressSanitizer", "runtime error", "LeakSanitizer") if m in p.stderr]
        assert p.returncode == 0 and not bad and p.stdout.startswith("ok"), (p.returncode, p.stderr[-3000:])
        raw = np.fromfile(fout, np.uint32)
        px = w * h
        ref = oracle_mod.trace(c["n"], c["g0"], c["E"], c["grid"]["r0"], c["grid"]["pyr"], fr.pos, fr.nrm, fr.alb, eye)
        assert np.array_equal(raw[:4 * px], ref["diffuse"].view(np.uint32).ravel())
        assert np.array_equal(raw[4 * px:8 * px], ref["spec"].view(np.uint32).ravel())
        assert np.array_equal(raw[8 * px:9 * px], ref["steps_px"].ravel())
        assert int(raw[9 * px:].view(np.uint64)[0]) == ref["cone_steps"]


# ---------------------------------------------------------------------------
# B.3  the apertures of the step-table tests hit what they claim
# ---------------------------------------------------------------------------
def test_aperture_step_counts():
    """t = 1; D = max(1, 2 tau t); t += 0.5 D while t <= n sqrt3 in binary32.  A 64-row table
    holds at most 63 steps and the sentinel: the 63-step aperture is the last that fits."""
    t63, t64, t65 = (TI.tau_with_steps(k, 32) for k in (63, 64, 65))
    assert TI.spec_steps(t63, 32) == 63 and TI.spec_steps(t64, 32) == 64 and TI.spec_steps(t65, 32) == 65
    assert t63 > t64 > t65 > 0.02
    up = lambda v: float(np.nextafter(F(v), F(2)))
    assert TI.spec_steps(up(t63), 32) == 62 and TI.spec_steps(up(t64), 32) == 63 and TI.spec_steps(up(t65), 32) == 64
    # the searched values are the upper ends of their ranges; mid-range decimals land in the same ranges
    assert [TI.spec_steps(t, 32) for t in (0.03792, 0.03693, 0.03594)] == [63, 64, 65]
    assert TI.spec_steps(0.02, 32) == 89 and TI.spec_steps(0.02, 16) == 54
    # values outside [TAU_MIN, TAU_MAX] clamp onto the end keys
    assert TI.spec_steps(0.001, 32) == TI.spec_steps(-3.0, 32) == 89
    assert TI.spec_steps(2.5, 32) == TI.spec_steps(40.0, 32) == TI.spec_steps(1.0, 32)
    # the same recurrence through spec_ref's scalar binary32 arithmetic
    for tau, n, want in ((t63, 32, 63), (t64, 32, 64), (t65, 32, 65), (0.02, 32, 89), (0.02, 16, 54)):
        tau2, tmax, t, k = spec_ref.f32(2.0 * spec_ref.f32(tau)), spec_ref.f32(n * spec_ref.SQRT3), 1.0, 0
        while t <= tmax:
            t = spec_ref.f32(t + spec_ref.f32(0.5 * max(1.0, spec_ref.f32(tau2 * t))))
            k += 1
        assert k == want, (tau, n, k)
    first, second = TI.aperture_sets(32)
    keys = lambda vs: {float(np.fmin(np.fmax(F(v), F(spec_ref.TAU_MIN)), F(1))) for v in vs}
    # twelve values on eight keys fill the eight slots exactly; the second set then meets a full cache
    assert len(keys(first)) == 8 and len(keys(second)) == 12 and not keys(first) & keys(second)
