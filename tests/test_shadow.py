"""Cone-traced soft shadows without a GPU: the boundary declares and binds the two functions
of include/vct_shadow.h, and the reference the GPU tests compare against
(tests/shadow_ref.py, a numpy restatement of vct_spec.h "shadow cones") has an exact fmaf,
reproduces spec_ref's A.6 march for cones that are never limited, gives the closed-form
answers, and covers the input classes the GPU tests rely on.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import lights_ref
import shadow_ref
import spec_ref
from lights_ref import bits_equal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def gbuffer(n):
    """The CPU G-buffer of the shared inputs: Cornell from (0, 0, 4) at shadow_ref.FRAMES[n]."""
    from vct import scenes
    from vct.camera import Camera
    w, h = shadow_ref.FRAMES[n]
    return scenes.raycast_numpy(lights_ref.cornell(n)["scene"], Camera(position=(0.0, 0.0, 4.0)), w, h)


def check_coverage(n, ref=None):
    """Over the marched (soft, not skipped) pairs of the shared inputs: every end class at
    least 10 %, the penumbra (0.05 < V < 0.95) at least 15 %, V == 1 exactly at least 10 %."""
    if ref is None:
        pos, nrm, _ = gbuffer(n)
        ref = shadow_ref.reference(n, pos, nrm)
    cov = shadow_ref.coverage(ref)
    print(n, cov)
    assert cov["pairs"] > 0
    for cls in ("alpha stop", "light reached", "left grid"):
        assert cov[cls] >= 0.10, (n, cls, cov)
    assert cov["penumbra"] >= 0.15, (n, cov)
    assert cov["lit"] >= 0.10, (n, cov)
    return cov


# ---- fmaf ---------------------------------------------------------------------------------
def test_fmaf_equals_the_scalar_one_on_random_triples():
    rng = np.random.default_rng(11)
    m = 100000
    tri = (rng.standard_normal((3, m)) * np.exp2(rng.integers(-12, 13, (3, m)))).astype(F)
    tri[2, ::3] = -(tri[0, ::3].astype(np.float64) * tri[1, ::3]).astype(F)      # cancellation
    tri[:, ::101] = 0.0
    got = shadow_ref.fmaf(tri[0], tri[1], tri[2])
    assert got.dtype == np.float32
    want = np.array([spec_ref.fmaf(float(a), float(b), float(c)) for a, b, c in tri.T], F)
    assert bits_equal(got, want)
    assert not bits_equal(got, tri[0] * tri[1] + tri[2])                          # the fused result differs somewhere


def test_fmaf_on_binary32_midpoints():
    """a * b = 1 + 2^-11 + 2^-24 sits exactly between two binary32 values; c decides the
    side although the binary64 sum cannot hold it (the TwoSum / round-to-odd case)."""
    a = F(1.0) + F(2.0 ** -12)
    lo, hi = F(1.0) + F(2.0 ** -11), np.nextafter(F(1.0) + F(2.0 ** -11), F(2.0))
    assert float(a) * float(a) == (float(lo) + float(hi)) / 2
    cases = []
    for e in (-30, -40, -60, -100, -120):
        cases += [(a, a, F(2.0 ** e), hi), (a, a, -F(2.0 ** e), lo)]
    cases.append((a, a, F(0.0), lo))                                             # the tie itself: to even (lo)
    assert int(lo.view(np.uint32)) & 1 == 0
    for sc in (F(2.0 ** -20), F(2.0 ** 30), F(-2.0)):                            # scaled and mirrored: powers of two
        cases += [(a * sc, a, c * sc, r * sc) for _, _, c, r in cases[:11]]
    A, B, C_, R = (np.array(v, F) for v in zip(*cases))
    got = shadow_ref.fmaf(A, B, C_)
    assert bits_equal(got, R)
    assert bits_equal(got, np.array([spec_ref.fmaf(float(x), float(y), float(z)) for x, y, z in zip(A, B, C_)], F))


# ---- the march against spec_ref's A.6 ----------------------------------------------------------
@pytest.mark.parametrize("aniso", [True, False])
def test_unlimited_cones_are_the_a6_march(oracle_mod, aniso):
    """A directional light never limits its cone: alpha bits and step counts equal
    spec_ref.Tracer.march (32 cones per setting, 64 in all; apertures across the clamp)."""
    n = 16
    c = lights_ref.cornell(n)
    level0 = c["level0"]
    mips = oracle_mod.pyramid_levels(n, oracle_mod.build_mips(n, level0, aniso), aniso)
    tracer = spec_ref.Tracer(n, c["g0"], c["E"], level0, mips, aniso)
    alpha = shadow_ref.cornell_alpha(n, aniso)
    pos, nrm, _ = gbuffer(n)
    fy, fx = np.nonzero(pos[..., 3] != 0)
    P, N = pos[fy, fx, :3], nrm[fy, fx, :3]
    q = (P - np.array(c["g0"], F)[None, :]) * (F(n) / F(c["E"])) + N
    Lc = lights_ref.prepare(c["lights"][-1], n, c["g0"], c["E"])
    l, f, ndl, t_lim, cls = lights_ref.evaluate(Lc, q, N)
    k = np.flatnonzero(cls["walk"])
    k = k[:: max(k.size // 32, 1)][:32]
    assert k.size == 32 and np.all(np.isinf(t_lim[k]))
    taus = [0.05, 0.2, spec_ref.TAU_MIN, 0.3, 1.0, 0.1, 0.5, 0.03]
    seen_alpha = 0
    for i, tau in enumerate(taus):
        sel = k[i::len(taus)]
        a, steps, end = shadow_ref.march(alpha, n, aniso, q[sel], l[sel], t_lim[sel], float(tau))
        for r, idx in enumerate(sel):
            res, st = tracer.march([float(v) for v in q[idx]], [float(v) for v in l[idx]], float(tau))
            assert F(res[3]).view(np.uint32) == a[r].view(np.uint32), (aniso, tau, idx)
            assert st == steps[r], (aniso, tau, idx)
            assert end[r] != shadow_ref.END_REACHED
            seen_alpha += int(end[r] == shadow_ref.END_ALPHA)
    assert seen_alpha > 0


# ---- closed forms ---------------------------------------------------------------------------
def _grid(n, a):
    level0 = np.zeros((n, n, n, 4), F)
    level0[..., 3] = a
    return shadow_ref.alpha_pyramid(n, level0, True)


def _cones(m, n, seed):
    rng = np.random.default_rng(seed)
    o = (rng.random((m, 3)) * (n - 4) + 2).astype(F)
    d = rng.standard_normal((m, 3)).astype(F)
    d = (d / np.sqrt((d * d).sum(axis=1, dtype=F))[:, None]).astype(F)
    return o, d


def test_known_answers(oracle_mod):
    n = 8
    o, d = _cones(40, n, 1)
    inf = np.full(40, np.inf, F)
    # an empty grid: V = 1 and no cone ends on alpha
    for tau in (0.02, 0.3):
        a, steps, end = shadow_ref.march(_grid(n, 0.0), n, True, o, d, inf, tau)
        assert not a.view(np.uint32).any() and np.all(end == shadow_ref.END_LEFT) and np.all(steps >= 1)
        assert np.all(shadow_ref.visibility(a) == 1.0)
        far = np.full(40, 3.25, F)       # ... or reaches its light first
        a, steps2, end = shadow_ref.march(_grid(n, 0.0), n, True, o, d, far, tau)
        assert np.all(end[steps2 < steps] == shadow_ref.END_REACHED) and (steps2 < steps).any()
    # t_lim <= 1: the light is reached before the first sample
    for t_lim in (1.0, 0.25):
        a, steps, end = shadow_ref.march(_grid(n, 1.0), n, True, o, d, np.full(40, t_lim, F), 0.1)
        assert not steps.any() and np.all(end == shadow_ref.END_REACHED) and np.all(shadow_ref.visibility(a) == 1.0)
    # level 0 of alpha 1 everywhere: tau 0.05 samples level 0 alone (D = 1) at t = 1, inside
    # the grid the trilinear weights sum to a >= 0.95, and V = 0 after that one sample
    a, steps, end = shadow_ref.march(_grid(n, 1.0), n, True, o, d, inf, 0.05)
    assert np.all(steps == 1) and np.all(end == shadow_ref.END_ALPHA)
    assert np.all(a >= F(0.95)) and not shadow_ref.visibility(a).view(np.uint32).any()
    # V itself: one correctly rounded divide
    assert shadow_ref.visibility(F(0.5)) == F(1.0) - F(0.5) / F(0.95)
    assert shadow_ref.visibility(F(0.95)) == 0 and shadow_ref.visibility(F(0.0)) == 1
    # the clamp
    assert shadow_ref.clamp_tau(0.001) == float(F(0.02)) and shadow_ref.clamp_tau(7.0) == 1.0
    assert shadow_ref.clamp_tau(0.3) == float(F(0.3))


def test_hard_lights_are_the_walk_and_the_composite(oracle_mod):
    """tan_half = 0 gives lights_ref.walk's V, and the composite over those planes is
    lights_ref.composite bit for bit."""
    n = 16
    c = lights_ref.cornell(n)
    g = c["grid"]
    pos, nrm, alb = gbuffer(n)
    lights = shadow_ref.lights_for(n)
    ref = shadow_ref.reference(n, pos, nrm, tan_half=[0.0] * len(lights))
    assert ref["steps"] == 0 and set(np.unique(ref["vis"]).tolist()) == {0.0, 1.0}
    occ = g["albedo_occ"][..., 3] != 0
    fy, fx = np.nonzero(pos[..., 3] != 0)
    q = (pos[fy, fx, :3] - np.array(c["g0"], F)[None, :]) * (F(n) / F(c["E"])) + nrm[fy, fx, :3]
    for j, light in enumerate(lights):
        l, f, ndl, t_lim, cls = lights_ref.evaluate(lights_ref.prepare(light, n, c["g0"], c["E"]), q, nrm[fy, fx, :3])
        k = np.flatnonzero(cls["walk"])
        V, _ = lights_ref.walk(occ, q[k], l[k], t_lim[k])
        want = np.zeros(pos.shape[:2], F)
        want[fy[k], fx[k]] = V
        assert bits_equal(ref["vis"][j], want), j
    rng = np.random.default_rng(5)
    D, S = rng.random(pos.shape).astype(F), (rng.random(pos.shape) * 0.2).astype(F)
    got = shadow_ref.composite(n, c["g0"], c["E"], pos, nrm, alb, D, S, lights, ref["vis"])
    assert bits_equal(got, lights_ref.composite(n, c["g0"], c["E"], g["albedo_occ"], pos, nrm, alb, D, S, lights))
    soft = shadow_ref.reference(n, pos, nrm)
    assert not bits_equal(shadow_ref.composite(n, c["g0"], c["E"], pos, nrm, alb, D, S, lights, soft["vis"]), got)
    assert bits_equal(soft["vis"][-1], ref["vis"][-1])                           # the last light is hard in both


@pytest.mark.parametrize("n", [8, 16, 32, 64])
def test_coverage_of_the_gpu_inputs(oracle_mod, n):
    check_coverage(n)


# ---- boundary ----------------------------------------------------------------------------------
def test_header_declares_shadow_functions():
    src = open(os.path.join(REPO, "include", "vct_shadow.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"vct_status\s+vct_shadow_cones_device\s*\(\s*vct_ctx\s*\*", code)
    assert re.search(r"vct_status\s+vct_composite_shadowed_device\s*\(\s*vct_ctx\s*\*", code)
    vct_h = open(os.path.join(REPO, "include", "vct.h")).read()
    assert '#include "vct_shadow.h"' in vct_h and '#include "vct_lights.h"' in vct_h
    assert re.search(r"#define\s+VCT_ABI_VERSION\s+1\b", vct_h)
    assert "shadow cones" in open(os.path.join(REPO, "include", "vct_spec.h")).read()


def test_binding_lists_them_and_hip_library_exports_them():
    import ctypes as C
    from vct import Context, VctLight, _lib
    assert set(_lib.SHADOW_EXTENSIONS) == {"vct_shadow_cones_device", "vct_composite_shadowed_device"}
    assert set(_lib.LIGHT_EXTENSIONS) == {"vct_inject_lights", "vct_composite_lights_device"}      # unchanged
    assert set(_lib.EXTENSIONS) == {"vct_inject_bounces", "vct_bounce_sources"}
    assert not set(_lib.SHADOW_EXTENSIONS) & (set(_lib.EXPORTS) | set(_lib.EXTENSIONS) | set(_lib.LIGHT_EXTENSIONS))
    assert len(_lib.EXPORTS) == 52 and "vct_composite_device" in _lib.EXPORTS                       # untouched
    assert callable(Context.shadow_cones_device) and callable(Context.composite_shadowed_device)
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vct_[a-z0-9_]+)", out))
    assert set(_lib.SHADOW_EXTENSIONS) <= exported and "vct_debug_shadow" in exported
    assert lib.vct_abi_version() == 1
    # VCT_EINVAL for a NULL ctx, no device needed
    one, th = (VctLight * 1)(), (C.c_float * 1)(0.1)
    assert _lib.bind_shadow_extension(lib, "vct_shadow_cones_device")(None, None, None, 4, 4, one, 1, th, None, None) == 1
    assert _lib.bind_shadow_extension(lib, "vct_composite_shadowed_device")(None, None, None, None, None, None, 4, 4,
                                                                            None, 0, None, None, None) == 1


def test_library_without_them_still_loads(oracle_mod):
    import ctypes as C
    from vct import _lib
    cpu = _lib.bind(C.CDLL(oracle_mod.CPU_BACKEND))
    for name in _lib.SHADOW_EXTENSIONS:
        assert not hasattr(cpu, name)
        with pytest.raises(AttributeError, match=name):
            _lib.bind_shadow_extension(cpu, name)
