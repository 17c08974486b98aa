"""include/vct_env.h without a GPU: tests/env_ref.py (the numpy restatement of vct_spec.h
"environment sky") against the properties the rule is written for -- the box mips, a float64
evaluation of the same formulas, seamlessness over the fold, the edges and the corners of the
square, bit-exact constants, hand-computed records -- then the input rules, the header's
literals, the bindings, vct.env's host helpers and the host's --env parser.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import env_ref as ER
import light_inputs as LI
import sky_ref
import spec_ref
from lights_ref import bits_equal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "voxel-based-global-illumination_amd", "build", "vct_headless")
F = np.float32
SIZES = (1, 2, 8, 64)
EPS24 = 2.0 ** -24
TAUS = (float("nan"), -1.0, 0.0, float(spec_ref.TAU_MIN), 0.3, 10.0, float("inf"))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _level_tau(S, j):
    """The tau whose level is exactly j: tau * S = 2^j."""
    return F(2.0 ** j / S)


def lookup_bound(Sj, rng_):
    """|float32 - float64| of one lookup at a level of Sj texels.  p * 0.5 + 0.5 carries the
    roundings of dot3 (3), s, the divide, the fold and its own (at most 4 * 2^-24 absolute, the
    operands being <= 1), u = that * S_j - 0.5 one more ulp of S_j: |du| <= 5 S_j 2^-24 per axis.
    The bilinear's slope per texel is at most the texel range, on two axes; its own fmafs and
    the level blend add a few ulp of the range."""
    return (10.0 * Sj + 4.0) * EPS24 * rng_


# ---- 1. mips -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
def test_mips_box_rule_and_means(S):
    m0 = ER.random_map(S, seed=S)
    pyr = ER.mips(m0)
    lg = S.bit_length() - 1
    assert len(pyr) == lg + 1 and all(pyr[j].shape == (S >> j, S >> j, 4) for j in range(lg + 1))
    assert bits_equal(pyr[0], m0)
    for j in range(lg):
        src, dst = pyr[j], pyr[j + 1]
        for y in range(dst.shape[0]):
            for x in range(dst.shape[1]):
                a00, a10, a01, a11 = src[2 * y, 2 * x], src[2 * y, 2 * x + 1], src[2 * y + 1, 2 * x], src[2 * y + 1, 2 * x + 1]
                want = ((a00 + a10) + (a01 + a11)) * F(0.25)
                assert want.dtype == np.float32 and bits_equal(dst[y, x], want)
    mean0 = pyr[0].astype(np.float64).mean(axis=(0, 1))
    for j in range(1, lg + 1):
        # two adds on a path per level, each within 2^-24 relative of a partial sum <= 4 * max
        err = np.abs(pyr[j].astype(np.float64).mean(axis=(0, 1)) - mean0).max()
        assert err <= 2 * j * EPS24, (j, err)
    # a constant is that constant at every level
    c = ER.mips(ER.constant_map(S, (0.3, 1.7, 1e-3), 0.25))
    assert all(bits_equal(l, np.broadcast_to(np.array([0.3, 1.7, 1e-3, 0.25], F), l.shape)) for l in c)


# ---- 2. the lookup against float64 ---------------------------------------------------------------------
@pytest.mark.parametrize("S", (8, 64))
def test_lookup_against_float64(S):
    """20 000 random unit directions and the texel-centre directions, random apertures, a random
    map in [0, 1), identity and tilted frames; no direction left out.  Measured on the CPU:
    S = 64: 3.2e-6 (identity), 3.0e-6 (tilted); S = 8: 4.7e-7; the bound (3.8e-5, 5.0e-6) is lookup_bound's."""
    rng = np.random.default_rng(5)
    pyr = ER.mips(ER.random_map(S, seed=3))
    for env in (ER.IDENTITY, ER.tilted(scale=1.0)):
        d = np.concatenate([_unit(rng, 20000), ER.world_dirs(env, ER.texel_dirs(S)).reshape(-1, 3).astype(F)])
        tau = np.concatenate([np.zeros(10000, F), rng.random(d.shape[0] - 10000).astype(F) * F(1.2)])
        got, m = ER.lookup(pyr, env, d, tau)
        want = ER.lookup64(pyr, env, d, tau)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"S={S} max |f32 - f64| = {err:.3e}, bound {lookup_bound(S, 1.0):.3e}")
        assert err <= lookup_bound(S, 1.0)
        assert (m >= 0).all() and (m <= S.bit_length() - 1).all() and len(np.unique(m.astype(int))) == S.bit_length()
    # at the texel centres, level 0 returns the texel itself to the rounding of u
    env = ER.IDENTITY
    got, _ = ER.lookup(pyr, env, ER.texel_dirs(S).reshape(-1, 3).astype(F), F(0))
    assert np.abs(got - pyr[0][..., :3].reshape(-1, 3)).max() <= lookup_bound(S, 1.0)


# ---- 3. seamlessness -------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
def test_no_seam_at_any_level(S):
    """Pairs of directions 2^-20 apart across the z = 0 fold, across the four edges of the square
    (map-space x = 0 or y = 0 with z < 0), at the edge midpoints (+-x, +-y) and around the
    corners (-z): each pair's points lie within 2 * 2^-20 of each other or of a common edge, u
    moves by at most S_j * 2^-20 per axis, and the fold rule makes the edge values agree."""
    e = 2.0 ** -20
    rng = np.random.default_rng(11)
    pyr = ER.mips(ER.random_map(S, seed=7))
    ang = rng.random(256) * 2 * np.pi
    c, s = np.cos(ang), np.sin(ang)
    z = -np.abs(s)                                                    # (c, z) is a unit vector of the lower half
    pairs = [(np.stack([c, s, np.full(256, e)], 1), np.stack([c, s, np.full(256, -e)], 1)),           # the fold
             (np.stack([np.full(256, e), c, z], 1), np.stack([np.full(256, -e), c, z], 1)),           # top / bottom edge
             (np.stack([c, np.full(256, e), z], 1), np.stack([c, np.full(256, -e), z], 1))]           # left / right edge
    for ax in (0, 1):                                                                                # edge midpoints
        for sg in (1.0, -1.0):
            quad = []
            for s1 in (e, -e):
                for s2 in (e, -e):
                    d = np.zeros(3)
                    d[ax], d[1 - ax], d[2] = sg, s1, s2
                    quad.append(d)
            pairs += [(np.array([quad[0]]), np.array([q])) for q in quad[1:]]
    corner = [np.array([[s1, s2, -1.0]]) for s1 in (e, -e) for s2 in (e, -e)]                        # the corners
    pairs += [(corner[0], q) for q in corner[1:]]
    for j in range(S.bit_length()):
        Sj = S >> j
        lv = pyr[j][..., :3]
        rng_ = float(lv.max() - lv.min())
        tol = 2.0 * Sj * e * rng_ + 2.0 * lookup_bound(Sj, max(rng_, float(lv.max())))
        for a, b in pairs:
            a = (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(F)
            b = (b / np.linalg.norm(b, axis=1, keepdims=True)).astype(F)
            va, ma = ER.lookup(pyr, ER.IDENTITY, a, _level_tau(S, j))
            vb, _ = ER.lookup(pyr, ER.IDENTITY, b, _level_tau(S, j))
            assert (ma == j).all()
            assert np.abs(va - vb).max() <= tol, (S, j, float(np.abs(va - vb).max()), tol)


# ---- 4. a constant map ---------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (1, 2, 4, 8, 64))
def test_constant_map_is_exact(S):
    """Every direction of the hostile catalogue, every aperture of TAUS, two frames: c in every bit."""
    c = np.array([0.3, 1.7, 1e-3], F)
    pyr = ER.mips(ER.constant_map(S, c))
    d = np.array([x.d for x in LI.directions()], F)
    assert d.shape[0] > 300 and not np.isfinite(d).all()
    for env in (ER.IDENTITY, ER.tilted(scale=1.0), ER.Y_UP):
        for tau in TAUS:
            got, m = ER.lookup(pyr, env, d, F(tau))
            assert bits_equal(got, np.broadcast_to(c, got.shape)), (S, tau)
            assert np.isfinite(m).all()
    got, _ = ER.lookup(pyr, dict(ER.IDENTITY, scale=3.7), d, F(0.3))
    assert bits_equal(got, np.broadcast_to(c * F(3.7), got.shape))


# ---- 5. hand-written records -------------------------------------------------------------------------------
def _map2():
    m = np.zeros((2, 2, 4), F)
    for (y, x), v in {(0, 0): 1.0, (0, 1): 2.0, (1, 0): 4.0, (1, 1): 8.0}.items():
        m[y, x] = (v, 2 * v, 0.5 * v, 1.0)
    return m


def _rgb(v):
    return np.array([v, 2 * v, 0.5 * v], F)


def test_hand_records_s2():
    """S = 2 with texels 1, 2 / 4, 8 (row 0 = p.y = -1): +z sees all four; -z folds onto the corner
    (1, 1), whose taps are the four texels again; +-x and +-y see the two texels of their side."""
    pyr = ER.mips(_map2())
    assert bits_equal(pyr[1][0, 0, :3], _rgb(3.75))
    cases = {(0, 0, 1): 3.75, (0, 0, -1): 3.75, (1, 0, 0): 5.0, (-1, 0, 0): 2.5, (0, 1, 0): 6.0, (0, -1, 0): 1.5,
             (0, 0, 7.5): 3.75, (3e-20, 0, 0): 5.0,                       # never normalised: only the L1 ratio counts
             (0.5, 0.5, 0.0): 8.0, (0.5, 0.5, -0.0): 8.0,                 # on the fold: u = 1 exactly, the texel (1, 1)
             (-0.5, 0.5, 0.0): 4.0, (0.5, -0.5, -0.0): 2.0, (-0.25, -0.25, 0.0): 1.0}
    for d, v in cases.items():
        got, m = ER.lookup(pyr, ER.IDENTITY, [d], F(0))
        assert bits_equal(got[0], _rgb(v)) and m[0] == 0, (d, got)
    # zero, NaN and infinite directions: the mean texel, whatever tau; m is still step 3's
    for d in ((0, 0, 0), (-0.0, 0.0, -0.0), (np.nan, 0, 1), (0, np.inf, 0), (-np.inf, 1, 1), (3e38, 3e38, 3e38)):
        for tau, m_want in ((0.0, 0.0), (np.nan, 0.0), (0.5, 0.0), (1.0, 1.0), (np.inf, 1.0)):
            got, m = ER.lookup(pyr, dict(ER.IDENTITY, scale=2.0), [d], F(tau))
            assert bits_equal(got[0], _rgb(7.5)) and m[0] == m_want, (d, tau, got, m)
    # the 90 degree frame: the map's +z is the world's +y, its +y the world's -z
    for d, v in {(0, 1, 0): 3.75, (0, -1, 0): 3.75, (1, 0, 0): 5.0, (0, 0, -1): 6.0, (0, 0, 1): 1.5}.items():
        got, _ = ER.lookup(pyr, ER.Y_UP, [d], F(0))
        assert bits_equal(got[0], _rgb(v)), (d, got)
    # tau >= 1 is the last level; in between, one fmaf of the two levels
    got, m = ER.lookup(pyr, ER.IDENTITY, [(1, 0, 0)], F(1.0))
    assert bits_equal(got[0], _rgb(3.75)) and m[0] == 1
    got, m = ER.lookup(pyr, ER.IDENTITY, [(1, 0, 0)], F(0.75))          # x = 1.5
    fr = F(spec_ref.log2(1.5))
    assert m[0] == fr and bits_equal(got[0], ER.fmaf(fr, _rgb(3.75) - _rgb(5.0), _rgb(5.0)))


def test_hand_records_s4_level_boundaries():
    """S = 4, direction +z (p = 0): level 0 sees the four central texels, levels 1 and 2 the mean."""
    m0 = np.zeros((4, 4, 4), F)
    m0[..., :3] = 1.0
    m0[1:3, 1:3, :3] = np.array([[2.0, 4.0], [6.0, 8.0]], F)[..., None]
    pyr = ER.mips(m0)
    B0, B1 = F(5.0), F((12 * 1.0 + 20.0) / 16.0)
    assert bits_equal(pyr[2][0, 0, 0], B1) and pyr[2][0, 0, 0] == 2.0
    below = float(np.nextafter(F(0.5), F(0)))
    above = float(np.nextafter(F(0.5), F(1)))
    for tau in (0.0, 0.25, 0.5, 0.75, 1.0, 2.0, below, above, 0.25 + 2.0 ** -25):
        x = spec_ref.fminf(spec_ref.fmaxf(spec_ref.f32(tau * 4.0), 1.0), 4.0)
        mw = min(spec_ref.log2(x), 2.0)
        j0 = int(mw)
        fr = F(mw - j0)
        lv = [B0, B1, B1]
        want = lv[j0] if not (fr > 0 and j0 < 2) else ER.fmaf(fr, lv[j0 + 1] - lv[j0], lv[j0])
        got, m = ER.lookup(pyr, ER.IDENTITY, [(0, 0, 1)], F(tau))
        assert m[0] == F(mw) and bits_equal(got[0], np.full(3, want, F)), (tau, got, want)
    assert ER.lookup(pyr, ER.IDENTITY, [(0, 0, 1)], F(0.5))[1][0] == 1.0            # exactly level 1
    assert 0 < 1.0 - ER.lookup(pyr, ER.IDENTITY, [(0, 0, 1)], F(below))[1][0] < 1e-6
    # the vectorised log2 is spec_ref's
    xs = np.concatenate([np.linspace(1, 2048, 500), 2.0 ** np.arange(12), [1.4142135, 1.4142137, 2.8284268]]).astype(F)
    assert bits_equal(ER.log2_f32(xs), np.array([spec_ref.log2(float(v)) for v in xs], F))


# ---- 6. input rules, literals, helpers, the host ---------------------------------------------------------------
def test_input_rules():
    good = ER.random_map(4)
    assert ER.map_error(good) is None
    for v, what in ((np.nan, "non-finite"), (np.inf, "non-finite"), (-0.0, "negative"), (-1.0, "negative"),
                    (float(np.nextafter(F(2.0 ** 52), F(np.inf))), "above")):
        for ch in range(3):
            bad = good.copy()
            bad[2, 1, ch] = v
            assert what in ER.map_error(bad), (v, ch)
    ok = good.copy()
    ok[..., 3] = np.nan                                       # alpha is not checked
    ok[0, 0, :3] = (2.0 ** 52, 0.0, 1e-45)
    assert ER.map_error(ok) is None
    assert [S for S in range(0, 70) if ER.size_error(S) is None] == [1, 2, 4, 8, 16, 32, 64]
    assert ER.size_error(2048) is None and ER.size_error(4096) and ER.size_error(3)
    # the record
    assert ER.record_error(ER.IDENTITY) is None and ER.record_error(ER.tilted()) is None and ER.record_error(ER.Y_UP) is None
    mirrored = dict(ER.IDENTITY, frame=((1, 0, 0), (0, 1, 0), (0, 0, -1)))
    assert ER.record_error(mirrored) is None                 # handedness is not tested
    for scale, what in ((np.nan, "non-finite"), (np.inf, "non-finite"), (-0.0, "negative"), (-2.0, "negative"),
                        (2.0 ** 53, "above")):
        assert what in ER.record_error(dict(ER.IDENTITY, scale=scale))
    assert ER.record_error(dict(ER.IDENTITY, scale=0.0)) is None and ER.record_error(dict(ER.IDENTITY, scale=2.0 ** 52)) is None
    for fr in (((1 + 2e-6, 0, 0), (0, 1, 0), (0, 0, 1)), ((1, 2e-6, 0), (0, 1, 0), (0, 0, 1)), ((0, 0, 0),) * 3,
               ((np.nan, 0, 0), (0, 1, 0), (0, 0, 1)), ((1, 0, 0), (0, np.inf, 0), (0, 0, 1)), ((2, 0, 0), (0, 0.5, 0), (0, 0, 1))):
        assert ER.record_error({"frame": fr, "scale": 1.0}), fr
    within = {"frame": ((1 + 4e-7, 0, 0), (0, 1, 4e-7), (0, 0, 1)), "scale": 1.0}
    assert ER.record_error(within) is None


def test_literals_bindings_and_null_ctx():
    from vct import Context, VctEnvSky, _lib, env_sky
    env_h = open(os.path.join(REPO, "include", "vct_env.h")).read()
    spec_h = open(os.path.join(REPO, "include", "vct_spec.h")).read()
    vct_h = open(os.path.join(REPO, "include", "vct.h")).read()
    assert int(re.search(r"#define VCT_ENV_MAX_DIM (\d+)u", env_h).group(1)) == _lib.VCT_ENV_MAX_DIM == ER.MAX_DIM == 2048
    lim = float(re.search(r"#define VCT_ENV_TEXEL_LIMIT ([0-9.e+]+)f", spec_h).group(1))
    assert lim == _lib.VCT_ENV_TEXEL_LIMIT == float(ER.TEXEL_LIMIT) == 2.0 ** 52
    assert vct_h.index('#include "vct_voxview.h"') < vct_h.index('#include "vct_env.h"')
    assert re.search(r"#define\s+VCT_ABI_VERSION\s+1\b", vct_h) and vct_h.count('#include "vct_env.h"') == 1
    assert C.sizeof(VctEnvSky) == 40 and len(_lib.EXPORTS) == 52                 # vct.h's list is untouched
    for name in _lib.ENV_EXTENSIONS:
        assert re.search(r"\b%s\(" % name, env_h), name
        assert name not in _lib.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vct_[a-z0-9_]+)", out))
    assert set(_lib.ENV_EXTENSIONS) <= exported and {"vct_debug_env", "vct_debug_env_path", "vct_debug_env_mips"} <= exported
    lib = _lib.load()
    assert lib.vct_abi_version() == 1
    e = env_sky()
    assert [list(r) for r in e.frame] == [[1, 0, 0], [0, 1, 0], [0, 0, 1]] and e.scale == 1.0
    e = env_sky(ER.Y_UP["frame"], 2.5)
    assert list(e.frame[1]) == [0, 0, -1] and e.scale == 2.5
    B = _lib.bind_env_extension
    buf = (C.c_float * 16)()
    assert B(lib, "vct_set_env")(None, buf, 2) == 1 and B(lib, "vct_env_size")(None) == 0
    assert B(lib, "vct_env_download_level")(None, 0, buf) == 1
    assert B(lib, "vct_env_lookup_device")(None, C.byref(e), None, 0, None) == 1
    assert B(lib, "vct_env_cones_device")(None, None, None, 1, 1, C.byref(e), None, None, None) == 1
    assert B(lib, "vct_inject_env")(None, C.byref(e)) == 1
    assert B(lib, "vct_env_specular_device")(None, None, None, None, 1, 1, None, C.byref(e), None, None, None) == 1
    assert B(lib, "vct_env_background_device")(None, None, None, 1, 1, C.byref(e), None, None) == 1
    for m in ("set_env", "env_download_level", "env_lookup_device", "env_cones_device", "inject_env",
              "env_specular_device", "env_background_device"):
        assert callable(getattr(Context, m))
    with pytest.raises(AttributeError, match="vct_env.h"):
        B(C.CDLL(None), "vct_set_env")


def test_python_helpers():
    """vct.env: the octahedral layout round-trips, agrees with the reference's point of a
    direction, and the three helpers fill the square; from_sky at S = 64 looked up at level 0
    is the three-colour sky to the bilinear's error (measured 1.2e-2 and 1.7e-2; the bound, 8e-2: the texel
    centres around a direction lie within 3 * sqrt(2) * 2 / S radians of it -- the octahedral
    map stretches at most 3x -- and Sky is Lipschitz in the angle with the largest colour step)."""
    from vct import VctEnvSky, sky_light
    from vct.env import EnvMap, Y_UP, oct_decode, oct_encode, texel_dirs
    rng = np.random.default_rng(2)
    d = _unit(rng, 4000).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert np.abs(oct_decode(oct_encode(d)) - d).max() < 1e-12
    p32, ok = ER.oct_point(ER.IDENTITY, d.astype(F))
    assert ok.all() and np.abs(p32 - oct_encode(d)).max() < 1e-6
    assert bits_equal(ER.texel_dirs(8) @ np.array(Y_UP, np.float64), texel_dirs(8))
    assert np.allclose(texel_dirs(4, ER.IDENTITY["frame"])[0, 0], oct_decode((-0.75, -0.75)))
    # from_function / the record
    m = EnvMap.from_function(lambda dd: np.stack([dd[..., 1] > 0, dd[..., 0] > 0, dd[..., 2] > 0], -1) * 2.0, 16, scale=1.5)
    assert m.size == 16 and m.texels.shape == (16, 16, 4) and m.texels.dtype == np.float32 and (m.texels[..., 3] == 1).all()
    assert ER.map_error(m.texels) is None and isinstance(m.record, VctEnvSky) and m.record.scale == 1.5
    assert (m.texels[4:12, 4:12, 0].mean() > 1.5) and m.texels[0, 0, 0] == 0                 # +y is the inner diamond
    assert ER.record_error({"frame": m.frame, "scale": m.scale}) is None
    with pytest.raises(ValueError):
        EnvMap(np.zeros((3, 3, 4), F))
    # from_sky
    S = 64
    for sky in (sky_ref.SKY, sky_ref.SKY_TILTED):
        em = EnvMap.from_sky(sky, S)
        em2 = EnvMap.from_sky(sky_light(sky["zenith"], sky["horizon"], sky["ground"], sky["up"]), S)
        assert np.abs(em.texels - em2.texels).max() < 1e-6
        pyr = ER.mips(em.texels)
        dirs = _unit(rng, 20000)
        got, _ = ER.lookup(pyr, {"frame": em.frame, "scale": 1.0}, dirs, F(0))
        want = sky_ref.sky_color(dirs, sky)
        cols = np.array([sky[k] for k in ("zenith", "horizon", "ground")])
        step = max(np.abs(cols[0] - cols[1]).max(), np.abs(cols[2] - cols[1]).max())
        err = float(np.abs(got - want).max())
        print(f"from_sky S={S}: max |Env - Sky| = {err:.3e}, bound {3 * np.sqrt(2) * 2 / S * step:.3e}")
        assert err <= 3 * np.sqrt(2) * 2 / S * step
    # from_equirect: a panorama that is a function of the direction comes back as that function
    hh, ww = 64, 128
    lat = (np.arange(hh) + 0.5) / hh * np.pi
    lon = (np.arange(ww) + 0.5) / ww * 2 * np.pi                       # column 0 looks along -z
    dy = np.cos(lat)[:, None] * np.ones(ww)
    dx = np.sin(lat)[:, None] * np.sin(lon)[None, :]
    dz = -np.sin(lat)[:, None] * np.cos(lon)[None, :]
    img = np.stack([dx, dy, dz], -1) * 0.5 + 0.5
    em = EnvMap.from_equirect(img, 32)
    assert np.abs(em.texels[..., :3] - (texel_dirs(32) * 0.5 + 0.5)).max() < 2e-2
    assert ER.map_error(em.texels) is None


def test_host_env_parser(tmp_path):
    """vct_headless --env FILE[:SCALE]: S from the file size; any other size, an unreadable file
    or a bad SCALE is the usage error (exit 2) before anything is loaded; a good one gets as far
    as the missing model (exit 1)."""
    assert os.path.exists(EXE), "build the host with `make -C voxel-based-global-illumination_amd host`"
    good = tmp_path / "env8.f32"
    ER.random_map(8).tofile(good)
    odd = tmp_path / "odd.f32"
    np.zeros(8 * 8 * 4 - 1, F).tofile(odd)
    three = tmp_path / "three.f32"
    np.zeros(3 * 3 * 4, F).tofile(three)
    empty = tmp_path / "empty.f32"
    empty.write_bytes(b"")
    colon = tmp_path / "a:b.f32"
    ER.random_map(1).tofile(colon)

    def run(*flags):
        return subprocess.run([EXE, "none.obj", *flags], capture_output=True, text=True, timeout=60)
    for flags in (["--env", str(good)], [f"--env={good}:2.5"], ["--env", f"{good}:0", "--sky-view"], ["--env", str(colon)],
                  ["--env", f"{colon}:1e3"], ["--sky", "0.2,0.4,1", "--env", str(good), "--sky-view"]):
        p = run(*flags)
        assert p.returncode == 1 and "cannot open" in p.stderr and "--env" not in p.stderr, (flags, p.returncode, p.stderr)
    for flags, what in ((["--env", str(odd)], "bytes is not"), (["--env", str(three)], "bytes is not"),
                        (["--env", str(empty)], "bytes is not"), (["--env", str(tmp_path / "missing.f32")], "cannot open"),
                        ([f"--env={good}:-1"], "SCALE"), ([f"--env={good}:nan"], "SCALE"), ([f"--env={good}:inf"], "SCALE"),
                        (["--env"], "FILE[:SCALE]"), (["--env="], "FILE[:SCALE]")):
        p = run(*flags)
        assert p.returncode == 2 and "malformed --env" in p.stderr and what in p.stderr, (flags, p.returncode, p.stderr)
    p = run("--sky-view")
    assert p.returncode == 2 and "--sky-view needs --sky" in p.stderr
