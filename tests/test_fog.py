"""tests/fog_ref.py (the numpy restatement of vct_spec.h "volumetric fog") against closed forms,
the input rule, and the coverage conditions of the inputs tests/test_fog_gpu.py uses.  No GPU.
"""
import numpy as np
import pytest

import fog_ref as R
from lights_ref import bits_equal

F = np.float32


def _unit_grid(n):
    """A grid whose voxel is the world unit: g0 = 0, E = n (inv_h = 1)."""
    return (0.0, 0.0, 0.0), float(n)


def _ray4(rows):
    return np.array(rows, F).reshape(1, -1, 4)


def test_zero_density_is_the_identity():
    """sigma = 0: F = +0 and T = 1 exactly on every ray, and apply leaves a frame bit-identical."""
    n = 32
    g0, E = _unit_grid(n)
    rng = np.random.default_rng(5)
    S = rng.random((16, 16, 16, 4)).astype(F)
    ray4, _ = R.eye_rays(n, g0, E, (16.3, 12.1, 50.0), 24, 16)
    out = R.march(n, g0, E, R.fog(0.0, level=1, step=0.5), (16.3, 12.1, 50.0), ray4, S)
    assert out["steps"] > 0
    assert not out["fog4"][..., :3].view(np.uint32).any()
    assert (out["fog4"][..., 3] == 1.0).all()
    frame = (rng.random((16, 24, 4)) * 3).astype(F)
    lin, _ = R.apply(out["fog4"], frame)
    assert bits_equal(lin, frame)


def test_constant_volume_closed_form():
    """S = s everywhere, sigma_v ds = 2^-3, N whole steps.

    T: every step multiplies by 1 - 1/8 = 7/8 exactly; (7/8)^N = 7^N / 2^(3N) has a 24-bit
    numerator for N <= 8 (7^8 < 2^23), so T == (7/8)^N exactly there.
    F: T a is then exact too (a power of two times T).  The trilinear sample of a constant
    volume: each axis' weight pair (1 - w, w) sums to 1 within one rounding (u = 2^-24), the
    product of three pairs within (1 + u)^3, each corner weight (wx wy) wz adds two roundings,
    and the eight fmaf accumulations of same-signed terms add at most 8 u: S = s (1 + d),
    |d| <= 13 u.  The N compositing fmafs round once each, relative to a running sum that
    never exceeds F: |F - s (1 - T)| <= (13 + N) u s (1 - T) up to second order.  u |x| <= ulp(x),
    so the bound asserted is (16 + N) ulps of s (1 - T), second-order terms included.
    On rays whose samples sit on cell centres every weight is 0 or 1, S = s exactly, and for
    s = 1 every partial sum (8^k - 7^k) / 8^k is representable: F == 1 - T exactly."""
    n = 32
    g0, E = _unit_grid(n)
    f = R.fog(1.0 / 16.0, level=1, step=1.0)             # sigma_v = 1/16 per voxel, ds = 2
    assert R.sigma_v(f, n, E) * F(2.0) == F(0.125)
    for s in (1.0, 0.3):
        S = np.full((16, 16, 16, 4), s, F)
        for N in range(1, 9):
            ray4 = _ray4([[1.0, 0.0, 0.0, 4.0 + 2.0 * N]])
            # samples at x = 1 + 2 i; y = z = 17 are cell centres, y = 16.3, z = 16.7 are not
            for eye, aligned in (((-4.0, 17.0, 17.0), True), ((-4.0, 16.3, 16.7), False)):
                out = R.march(n, g0, E, f, eye, ray4, S)
                T, Fc = out["fog4"][0, 0, 3], out["fog4"][0, 0, :3]
                assert out["samples"][0, 0] == N and out["end"][0, 0] == R.END_SAMPLES
                assert T == F(0.875 ** N) and float(T) == 7.0 ** N / 8.0 ** N
                if aligned and s == 1.0:
                    assert (Fc == F(1.0) - T).all()
                want = float(F(s)) * (1.0 - float(T))
                ulp = float(np.spacing(F(want)))
                assert np.abs(Fc.astype(np.float64) - want).max() <= (16 + N) * ulp, (s, N, eye, Fc, want)


def test_axis_ray_from_outside_gets_the_closed_form_slab():
    n = 32
    g0, E = _unit_grid(n)
    o = R.origin(n, g0, E, (-4.0, 17.0, 9.5))
    d = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]], F)
    ln = np.array([np.inf, np.inf, 10.0], F)
    t0, t1, ok, null = R.slab(n, o, d, ln)
    assert ok.tolist() == [True, False, True] and not null.any()
    assert t0[0] == 4.0 and t1[0] == 36.0                      # (0 - o_x) / d_x, (n - o_x) / d_x
    assert t0[2] == 4.0 and t1[2] == 10.0                      # ended by its own length
    # the two zero components do not clip while o lies inside their slabs, and empty the ray otherwise
    o2 = R.origin(n, g0, E, (-4.0, 33.0, 9.5))
    assert not R.slab(n, o2, d[:1], ln[:1])[2][0]
    out = R.march(n, g0, E, R.fog(0.5, level=1), (-4.0, 17.0, 9.5), _ray4([[1, 0, 0, np.inf], [-1, 0, 0, np.inf],
                                                                              [0, 0, 0, 0], [np.nan, 0, 0, 1.0]]),
                  np.ones((16, 16, 16, 4), F))
    assert out["end"][0].tolist()[1:] == [R.END_EMPTY, R.END_NULL, R.END_NULL]
    assert bits_equal(out["fog4"][0, 1:], np.array([[0, 0, 0, 1]] * 3, F))
    assert out["entered"][0, 0] and np.isfinite(out["fog4"]).all()


def test_axis_whose_reciprocal_overflows_does_not_clip():
    """|d_c| <= 2^-128: 1 / d_c is +-inf, so the axis is treated as d_c == 0 -- it does not clip
    while o_c lies in [0, n] and empties the segment otherwise -- and no t is NaN.  The segment is
    the one of the same ray with those components exactly 0."""
    n = 32
    g0, E = _unit_grid(n)
    tiny = F(2.0 ** -130)
    with np.errstate(over="ignore"):
        assert tiny != 0 and np.isinf(F(1.0) / tiny)
    d = np.array([[1.0, tiny, -tiny], [1.0, 0.0, 0.0]], F)
    ln = np.array([np.inf, np.inf], F)
    o = R.origin(n, g0, E, (-4.0, 17.0, 9.5))
    t0, t1, ok, null = R.slab(n, o, d, ln)
    assert ok.all() and not null.any() and t0.tolist() == [4.0, 4.0] and t1.tolist() == [36.0, 36.0]
    assert not R.slab(n, R.origin(n, g0, E, (-4.0, 17.0, 32.5)), d, ln)[2].any()      # o_z outside its slab
    assert R.slab(n, R.origin(n, g0, E, (-4.0, 0.0, 32.0)), d, ln)[2].all()           # on the faces: inside
    # 2^-127 is the first denormal whose reciprocal is finite: that axis clips like any other
    d2 = np.array([[1.0, F(2.0 ** -127), 0.0]], F)
    assert np.isfinite(F(1.0) / d2[0, 1])
    t0, t1, ok, _ = R.slab(n, o, d2, ln[:1])
    assert ok[0] and t0[0] == 4.0 and t1[0] == 36.0 and np.isfinite([t0[0], t1[0]]).all()
    S = np.random.default_rng(2).random((16, 16, 16, 4)).astype(F)
    out = R.march(n, g0, E, R.fog(1.0 / 16.0, level=1), (-4.0, 17.0, 9.5), np.concatenate([d, ln[:, None]], 1).reshape(1, 2, 4), S)
    assert bits_equal(out["fog4"][0, 0], out["fog4"][0, 1]) and out["samples"][0, 0] == 16


@pytest.fixture(scope="module")
def cornell32(oracle_mod):
    return R.scene("cornell", 32)


def test_sun_through_the_skylight(cornell32):
    """A unit-albedo cell the sun reaches unoccluded holds VCT_FOG_PHASE * C exactly; a cell whose
    cone saturates (a >= VCT_ALPHA_STOP) holds +0."""
    sc = cornell32
    sun = sc["lights"][:1]
    C = np.array(sun[0].color, F)
    b = R.build(32, sc["g0"], sc["E"], sc["alpha"], True, R.fog(1.0, level=1), sun, [R.TAN])
    S = b["S"].reshape(-1, 4)
    V = b["V"][0]
    lit, dark = V == 1.0, V == 0.0
    print("sun cells: lit", int(lit.sum()), "dark", int(dark.sum()), "partial", int(((V > 0) & (V < 1)).sum()))
    assert lit.any() and dark.any()
    assert bits_equal(S[lit, :3], np.broadcast_to(R.PHASE * C, (int(lit.sum()), 3)))
    assert not S[dark].view(np.uint32).any()
    assert not S[:, 3].view(np.uint32).any()


def test_transmittance_never_rises(cornell32):
    sc = cornell32
    f = R.fog(3.0, (0.9, 0.8, 0.7), level=1, step=0.5)
    b = R.build(32, sc["g0"], sc["E"], sc["alpha"], True, f, sc["lights"], [R.TAN] * 3)
    ray4, _ = R.eye_rays(32, sc["g0"], sc["E"], R.EYE_IN, 24, 16)
    out = R.march(32, sc["g0"], sc["E"], f, R.EYE_IN, ray4, b["S"])
    tr = np.stack([np.ones_like(out["T_trace"][0])] + out["T_trace"])
    assert len(out["T_trace"]) > 4 and (np.diff(tr, axis=0) <= 0).all()
    assert (out["fog4"][..., :3] >= 0).all() and (out["fog4"][..., :3] > 0).any()


ILLEGAL = [
    dict(density=-0.0), dict(density=-1.0), dict(density=float("nan")), dict(density=float("inf")),
    dict(density=2.0 ** 20 * 1.5), dict(albedo=(0.5, -0.0, 0.5)), dict(albedo=(1.5, 0.5, 0.5)),
    dict(albedo=(0.5, 0.5, float("nan"))), dict(albedo=(-0.1, 0.5, 0.5)), dict(ambient=-1.0),
    dict(ambient=float("inf")), dict(ambient=float("nan")), dict(level=0), dict(level=4), dict(level=40),
    dict(step=0.2), dict(step=4.5), dict(step=float("nan")), dict(step=-1.0),
]


def test_input_rule():
    """Every illegal field of the table in vct_fog.h is refused by the validator the binding
    shares with the tests (n = 32: level 4 leaves 2 cells); the legal corners pass."""
    from vct import _lib
    base = dict(density=0.5, albedo=(0.9, 0.9, 0.9), ambient=0.0, level=2, step=1.0)
    check = lambda d: _lib.check_fog(d["density"], d["albedo"], d["ambient"], d["level"], d["step"], 32, 2.2)
    assert check(base) is None
    for legal in (dict(density=0.0), dict(density=2.0 ** 20), dict(albedo=(0.0, 1.0, 0.5)), dict(ambient=0.0),
                  dict(ambient=7.0), dict(level=1), dict(level=3), dict(step=0.25), dict(step=4.0)):
        assert check({**base, **legal}) is None, legal
    for bad in ILLEGAL:
        assert check({**base, **bad}) is not None, bad
    assert _lib.check_fog(2.0 ** 20, (1, 1, 1), 0.0, 1, 1.0, 32, 3e38) is not None     # density * E overflows


def test_coverage_of_the_gpu_inputs(oracle_mod):
    """The restatement alone, on the inputs of tests/test_fog_gpu.py: every class the GPU
    comparison is meant to exercise occurs.  Of the valid pixels' rays at most 60 % take fewer
    than two samples, over all cases together and in every case whose step is at most an
    eighth of the grid (a step of half the grid or more cannot give a ray two samples)."""
    import fog_inputs as I
    tot = dict(tstop=0, remainder=0, entered=0, missed=0, null=0, partial=0, range=0, cone=0, clamped=0)
    few = valid_all = 0
    for case in I.CASES:
        ref = I.reference(case)
        m, b = ref["march"], ref["build"]
        valid = ref["pos"][..., 3] != 0
        end = m["end"]
        c = dict(tstop=int((end == R.END_TSTOP).sum()),
                 remainder=int(((end == R.END_SAMPLES) & (m["last_len"] < m["ds"]) & (m["samples"] == m["N"])).sum()),
                 entered=int(m["entered"].sum()), missed=int((end == R.END_EMPTY).sum()),
                 null=int((end == R.END_NULL).sum()), partial=int(((b["V"] > 0) & (b["V"] < 1)).sum()),
                 range=int((b["skip"] == R.SKIP_RANGE).sum()), cone=int((b["skip"] == R.SKIP_CONE).sum()),
                 clamped=int(m["clamped"].sum()))
        if case.hostile:
            # every class of hostile pixel is in this frame's row 0, and the restatement gives each
            # the record the spec names: +0 for what is not a ray, a unit d and a finite len otherwise
            cls = I.hostile_classes(case)
            print(case.name, "hostile row", {k: cls.count(k) for k in I.HOSTILE_CLASSES})
            assert set(cls) == set(I.HOSTILE_CLASSES), sorted(set(I.HOSTILE_CLASSES) - set(cls))
            row, prow = ref["rays"][0], ref["pos"][0]
            for x, k in enumerate(cls):
                if k in ("eye", "nan_x", "nan_y", "nan_z", "posinf", "neginf", "big"):
                    assert not row[x].view(np.uint32).any(), (x, k, row[x])
                elif k in ("far", "near", "denorm"):
                    assert np.isfinite(row[x]).all() and row[x, 3] > 0, (x, k, row[x])
                elif prow[x, 3] != 0:                            # a hostile pos.w that counts as valid (NaN, 2, -1, denormal)
                    assert np.isfinite(row[x]).all() and row[x, 3] > 0, (x, k, row[x])
        short = int((m["samples"][valid] < 2).sum())
        print(case.name, c, "valid", int(valid.sum()), "under two samples", short)
        for k in tot:
            tot[k] += c[k]
        few += short
        valid_all += int(valid.sum())
        if m["ds"] <= case.n / 8 and valid.sum() > 1:
            assert short <= 0.6 * valid.sum(), case.name
    print("total", tot, "valid", valid_all, "under two samples", few)
    for k, v in tot.items():
        assert v > 0, k
    assert few <= 0.6 * valid_all
