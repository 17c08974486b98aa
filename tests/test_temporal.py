"""Temporal accumulation without a GPU: the boundary declares, binds and exports the functions of
include/vct_temporal.h, a library without them still loads, the host refuses a malformed
--temporal, and tests/temporal_ref.py (the numpy restatement the GPU tests compare with) has
the properties the spec states, on the scene, cameras and frame sizes the GPU tests use (CPU
caster G-buffers): the same camera reprojects every pixel onto itself, a constant stays
constant, a sequence gives its running mean, max_len = 1 returns the input, a poisoned history
resets exactly its reusers, a vanished motion vector resets, and the input rules.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_inputs as TI
import temporal_ref as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "voxel-based-global-illumination_amd", "build", "vct_headless")
NAMES = ("vct_temporal_default_params", "vct_temporal_accumulate_device")
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the boundary -----------------------------------------------------------------------------------
def test_header_and_spec_declare_the_functions():
    src = open(os.path.join(REPO, "include", "vct_temporal.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(rf"vct_status\s+{name}\s*\(\s*(const\s+)?vct_ctx\s*\*", code), name
    for text in ("VCT_TEMPORAL_DEFAULT_LEN 8u", "VCT_TEMPORAL_MAX_LEN     1024u", "not measured optima",
                 "VCT_MIXED_NORMAL_COS", "never waits", "no voxelization"):
        assert text in src, text
    vct_h = open(os.path.join(REPO, "include", "vct.h")).read()
    assert vct_h.count('#include "vct_temporal.h"') == 1
    assert vct_h.index('#include "vct_fog.h"') < vct_h.index('#include "vct_temporal.h"')
    assert re.search(r"#define\s+VCT_ABI_VERSION\s+1\b", vct_h)
    assert not any(name in vct_h for name in NAMES)
    spec = open(os.path.join(REPO, "include", "vct_spec.h")).read()
    block = spec.split("---- temporal accumulation", 1)[1]
    for text in ("X16 = (int)floorf(fx * 16.0f + 0.5f)", "normal_cos", "plane_eps", "reset_offscreen", "reset_rejected",
                 "out = H + (cur - H) * wk", "min(L, max_len - 1) + 1", "(0,0), (1,0), (0,1), (1,1)"):
        assert text in block, text


def test_binding_lists_them_and_hip_library_exports_them():
    from vct import Context, _lib
    from vct.temporal import History
    assert _lib.TEMPORAL_EXTENSIONS == NAMES
    assert not set(NAMES) & (set(_lib.EXPORTS) | set(_lib.MIXED_EXTENSIONS) | set(_lib.FOG_EXTENSIONS))
    for m in ("temporal_params", "temporal_accumulate_device"):
        assert callable(getattr(Context, m)), m
    assert callable(History.accumulate) and callable(History.reset)
    assert C.sizeof(_lib.VctTemporalParams) == 12
    assert (_lib.VCT_TEMPORAL_DEFAULT_LEN, _lib.VCT_TEMPORAL_MAX_LEN) == (T.DEFAULT_LEN, T.MAX_LEN)
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vct_[a-z0-9_]+)", out))
    assert set(NAMES) <= exported
    assert lib.vct_abi_version() == 1
    # VCT_EINVAL for a NULL ctx, no device needed
    assert _lib.bind_temporal_extension(lib, "vct_temporal_default_params")(None, None) == 1
    assert _lib.bind_temporal_extension(lib, "vct_temporal_accumulate_device")(None, None, None) == 1


def test_args_struct_matches_the_header():
    """The ctypes mirror has the C struct's layout: field order from the header's text, offsets
    from the natural alignment of an LP64 target."""
    from vct import _lib
    src = open(os.path.join(REPO, "include", "vct_temporal.h")).read()
    body = re.search(r"typedef struct vct_temporal_args \{(.*?)\} vct_temporal_args;", src, re.S).group(1)
    names = re.findall(r"(\w+)(?:\[4\])?\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _lib.VctTemporalArgs._fields_]
    A = _lib.VctTemporalArgs
    assert (A.width.offset, A.height.offset, A.pos4.offset, A.prev_cam.offset, A.n_planes.offset) == (0, 4, 8, 32, 56)
    assert (A.cur4.offset, A.hist4.offset, A.out4.offset, A.hist_len.offset, A.stats.offset) == (64, 96, 128, 160, 176)
    assert C.sizeof(A) == 184


def test_library_without_them_still_loads(oracle_mod):
    from vct import _lib
    cpu = _lib.bind(C.CDLL(oracle_mod.CPU_BACKEND))
    for name in NAMES:
        assert not hasattr(cpu, name)
        with pytest.raises(AttributeError, match=name):
            _lib.bind_temporal_extension(cpu, name)


@pytest.mark.parametrize("value", ["0", "1025", "-2", "2.0", "two", "", "2x", "4 ", "+3"])
def test_host_refuses_a_malformed_temporal_length(value):
    assert os.path.exists(EXE), "build the host with `make -C voxel-based-global-illumination_amd host`"
    for flags in (["--temporal", value], [f"--temporal={value}"]):
        p = subprocess.run([EXE, "none.obj"] + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "malformed --temporal" in p.stderr, (flags, p.returncode, p.stderr)


def test_host_accepts_temporal_before_it_needs_the_model():
    assert os.path.exists(EXE)
    for flags in (["--temporal", "1"], ["--temporal=1024"], ["--temporal", "8"]):
        p = subprocess.run([EXE, "none.obj"] + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "cannot open" in p.stderr, (flags, p.returncode, p.stderr)


# ---- helpers ----------------------------------------------------------------------------------------
def first_frame(gb, cur, **kw):
    """A frame without history."""
    return T.accumulate(gb[0], gb[1], cur, plane_eps=TI.plane_eps(), **kw)


def next_frame(gb, cur, cam, prev_gb, prev, **kw):
    return T.accumulate(gb[0], gb[1], cur, cam, prev_gb[0], prev_gb[1], prev["out"], prev["out_len"],
                        plane_eps=TI.plane_eps(), **kw)


# ---- the same camera --------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", TI.FRAMES)
def test_same_camera_reprojects_every_pixel_onto_itself(frame):
    """X16 = 16 x and Y16 = 16 y at every valid pixel, so the single tap weighs 256, H is the
    history bit for bit and out_len = min(len + 1, max_len)."""
    w, h = frame
    gb = TI.cpu_gbuffer("a", w, h)
    valid = gb[0][..., 3] != 0
    assert valid.any()
    fx, fy, ok = T.project(gb[0][..., :3], TI.cam_a(), w, h)
    assert ok[valid].all()
    X16 = np.floor(fx * F(16.0) + F(0.5)).astype(np.int64)
    Y16 = np.floor(fy * F(16.0) + F(0.5)).astype(np.int64)
    assert (X16 == 16 * np.arange(w)[None, :])[valid].all() and (Y16 == 16 * np.arange(h)[:, None])[valid].all()
    c0, c1 = TI.planes(1, w, h, 2), TI.planes(2, w, h, 2)
    r0 = first_frame(gb, c0)
    assert all(same(o[valid], c[valid]) for o, c in zip(r0["out"], c0))
    assert not any(bits(o[~valid]).any() for o in r0["out"])                  # background: +0
    assert np.array_equal(r0["out_len"], valid.astype(np.uint32))
    assert r0["stats"] == (int(valid.sum()), 0, int(valid.sum()), 0)
    r1 = next_frame(gb, c1, TI.cam_a(), gb, r0, max_len=3)
    assert r1["stats"] == (int(valid.sum()), int(valid.sum()), 0, 0)
    assert (r1["accepted"][valid] == 1).all() and all(t == [(y, x, 256)] for (y, x), t in r1["taps"].items())
    with np.errstate(all="ignore"):
        for o, c, hh in zip(r1["out"], c1, r0["out"]):                          # H = the history itself
            assert same(o[valid], (hh + (c - hh) * (F(1.0) / F(2.0)))[valid])
    r2 = next_frame(gb, c1, TI.cam_a(), gb, r1, max_len=3)
    r3 = next_frame(gb, c1, TI.cam_a(), gb, r2, max_len=3)
    for r, k in ((r1, 2), (r2, 3), (r3, 3)):
        assert np.array_equal(r["out_len"], np.where(valid, k, 0).astype(np.uint32))


# ---- a constant, a running mean, max_len = 1 --------------------------------------------------------
def test_constant_input_stays_that_constant():
    """2 * max_len frames of one constant plane: c + (c - c) * wk = c in every frame, for
    24-bit constants too (no product of the blend rounds: the only tap weighs 256)."""
    w, h = 13, 7
    gb = TI.cpu_gbuffer("a", w, h)
    valid = gb[0][..., 3] != 0
    cur = [np.full((h, w, 4), F(1.0) / F(3.0), F), np.full((h, w, 4), F(-1234.5678), F)]
    r = first_frame(gb, cur)
    for k in range(2, 2 * T.DEFAULT_LEN + 1):
        r = next_frame(gb, cur, TI.cam_a(), gb, r)
        assert all(same(o[valid], c[valid]) for o, c in zip(r["out"], cur)), k
        assert (r["out_len"][valid] == min(k, T.DEFAULT_LEN)).all()


def test_running_mean_within_the_rounding_bound():
    """c_1 .. c_k, k <= max_len, gives the arithmetic mean.  Bound: frame 1 is exact (a reset).
    Frame j computes a_j = a + (c_j - a) * wk with wk = fl(1 / j): with u = 2^-24 and every
    |value| <= M, the subtraction errs by at most 2 M u, the rounding of wk and of the product by
    2 M u / j each relative to a product of at most 2 M / j, and the addition by M u: at most
    (1 + 6 / j) M u <= 7 M u per frame.  An earlier error is carried with the factor
    (1 - 1 / j) <= 1, so after k frames |a_k - mean| <= 7 (k - 1) M u, second-order terms (below
    k^2 u^2 M) covered by the factor 1.001."""
    w, h, k = 13, 7, T.DEFAULT_LEN
    gb = TI.cpu_gbuffer("a", w, h)
    valid = gb[0][..., 3] != 0
    seq = [TI.planes(10 + j, w, h, 1) for j in range(k)]
    M = 4.0
    r = first_frame(gb, seq[0], max_len=k)
    for j in range(2, k + 1):
        r = next_frame(gb, seq[j - 1], TI.cam_a(), gb, r, max_len=k)
        mean = np.mean([s[0].astype(np.float64) for s in seq[:j]], axis=0)
        err = np.abs(r["out"][0].astype(np.float64) - mean)[valid].max()
        print(f"frame {j}: |a - mean| max {err:.3e}, bound {7 * (j - 1) * M * 2.0 ** -24 * 1.001:.3e}")
        assert err <= 7 * (j - 1) * M * 2.0 ** -24 * 1.001, j
    assert (r["out_len"][valid] == k).all()


def test_max_len_one_returns_the_input():
    w, h = 13, 7
    gb = TI.cpu_gbuffer("a", w, h)
    valid = gb[0][..., 3] != 0
    c0, c1 = TI.planes(3, w, h, 1), TI.planes(4, w, h, 1)
    r0 = first_frame(gb, c0, max_len=1)
    r1 = next_frame(gb, c1, TI.cam_a(), gb, r0, max_len=1)
    assert same(r1["out"][0][valid], c1[0][valid])
    assert np.array_equal(r1["out_len"], valid.astype(np.uint32))
    assert r1["stats"] == (int(valid.sum()), 0, 0, int(valid.sum()))           # counted as resets
    assert (r1["cause"][valid] == T.LENGTH_ONE).all()


# ---- the moved camera -------------------------------------------------------------------------------
_moved = {}


def moved(frame, n_planes=1):
    """CAM_A's reset frame followed by CAM_B's frame; computed once per size."""
    if (frame, n_planes) not in _moved:
        w, h = frame
        ga, gb = TI.cpu_gbuffer("a", w, h), TI.cpu_gbuffer("b", w, h)
        r0 = first_frame(ga, TI.planes(5, w, h, n_planes))
        r1 = next_frame(gb, TI.planes(6, w, h, n_planes), TI.cam_a(), ga, r0)
        _moved[(frame, n_planes)] = (ga, gb, r0, r1)
    return _moved[(frame, n_planes)]


@pytest.mark.parametrize("frame", TI.COVERED)
def test_moved_camera_shows_every_class(frame):
    """What the GPU's moved-camera test needs of CAM_A -> CAM_B: a quarter of the valid pixels
    reuse history through >= 2 accepted taps of different weights, pixels reset off screen and
    for want of a tap, a pixel mixes accepted and rejected taps, and a tap index is -1 or w."""
    ga, gb, r0, r1 = moved(frame)
    cov = T.coverage(r1)
    print(frame, cov, r1["stats"])
    T.check_moved_coverage(cov)
    assert set(np.unique(r1["cause"])) >= {0, T.PROJECTION, T.NO_TAP}
    reused = r1["cls"] == T.REUSED
    assert (r1["out_len"][reused] == 2).all() and (r1["out_len"][(r1["cls"] >= T.OFFSCREEN)] == 1).all()
    assert all(sum(bw for _, _, bw in t) <= 256 for t in r1["taps"].values())


def test_poisoned_history_resets_exactly_its_reusers():
    """A NaN (or Inf) in one history pixel, in one channel of one plane: the pixels with an
    accepted tap there reset (reset_rejected, out = cur), every other pixel keeps its bits."""
    frame = (32, 24)
    w, h = frame
    ga, gb, r0, r1 = moved(frame, 2)
    cur = TI.planes(6, w, h, 2)
    users = {}
    for (y, x), taps in r1["taps"].items():
        if r1["cls"][y, x] == T.REUSED:
            for Y, X, _ in taps:
                users.setdefault((Y, X), []).append((y, x))
    (Y, X), reusers = max(users.items(), key=lambda kv: len(kv[1]))
    assert len(reusers) >= 2
    for bad, plane, ch in ((np.nan, 1, 2), (np.inf, 0, 0), (-np.inf, 1, 3)):
        hist = [a.copy() for a in r0["out"]]
        hist[plane][Y, X, ch] = bad
        r = T.accumulate(gb[0], gb[1], cur, TI.cam_a(), ga[0], ga[1], hist, r0["out_len"], plane_eps=TI.plane_eps())
        hit = np.zeros((h, w), bool)
        for y, x in reusers:
            hit[y, x] = True
        assert (r["cls"][hit] == T.REJECTED).all() and (r["cause"][hit] == T.NON_FINITE).all()
        assert np.array_equal(r["cls"][~hit], r1["cls"][~hit])
        for p in range(2):
            assert same(r["out"][p][hit], cur[p][hit]) and same(r["out"][p][~hit], r1["out"][p][~hit])
            assert np.isfinite(r["out"][p]).all()
        assert (r["out_len"][hit] == 1).all() and np.array_equal(r["out_len"][~hit], r1["out_len"][~hit])
        assert r["stats"][3] == r1["stats"][3] + len(reusers)


def test_motion_without_a_previous_position_resets():
    """motion4 = the pixel's own position is the static case bit for bit; w = 0 resets that
    pixel (reset_offscreen) and no other; a NaN w is not 0."""
    frame = (32, 24)
    w, h = frame
    ga, gb, r0, r1 = moved(frame)
    cur = TI.planes(6, w, h, 1)
    motion = gb[0].copy()
    motion[..., 3] = 1
    r = next_frame(gb, cur, TI.cam_a(), ga, r0, motion=motion)
    assert same(r["out"][0], r1["out"][0]) and r["stats"] == r1["stats"]
    gone = np.zeros((h, w), bool)
    ys, xs = np.nonzero(r1["cls"] == T.REUSED)
    gone[ys[::5], xs[::5]] = True
    motion[gone, 3] = 0
    nan_w = (r1["cls"] == T.REUSED) & ~gone
    motion[nan_w, 3] = np.nan
    r = next_frame(gb, cur, TI.cam_a(), ga, r0, motion=motion)
    assert (r["cls"][gone] == T.OFFSCREEN).all() and (r["cause"][gone] == T.NO_MOTION).all()
    assert same(r["out"][0][gone], cur[0][gone]) and (r["out_len"][gone] == 1).all()
    assert same(r["out"][0][~gone], r1["out"][0][~gone]) and np.array_equal(r["cls"][~gone], r1["cls"][~gone])
    assert r["stats"] == (r1["stats"][0], r1["stats"][1] - int(gone.sum()), r1["stats"][2] + int(gone.sum()), r1["stats"][3])


def test_moving_box_with_and_without_motion():
    """The box of the GPU's moving-box test, on the CPU caster: without motion4 its pixels
    look up where they are now (the history of whatever was there: rejected by the plane test,
    or reused when the box's own face was there); with motion4 they look up where they were."""
    w, h = 32, 24
    g0 = TI.cpu_gbuffer("a", w, h, (0.0, 0.0, 0.0))
    g1 = TI.cpu_gbuffer("a", w, h, TI.BOX_T)
    motion, on_box = TI.box_motion(g1[0], TI.BOX_T)
    assert on_box.sum() >= 8 and (g1[0][..., 3] != 0)[~on_box].any()
    r0 = first_frame(g0, TI.planes(7, w, h, 1))
    cur = TI.planes(8, w, h, 1)
    plain = next_frame(g1, cur, TI.cam_a(), g0, r0)
    moved_ = next_frame(g1, cur, TI.cam_a(), g0, r0, motion=motion)
    print("box pixels", int(on_box.sum()), "reused without motion", int((plain["cls"][on_box] == T.REUSED).sum()),
          "with", int((moved_["cls"][on_box] == T.REUSED).sum()))
    assert (moved_["cls"][on_box] == T.REUSED).sum() > (plain["cls"][on_box] == T.REUSED).sum()
    assert (plain["cls"][on_box] == T.REJECTED).any()
    assert same(plain["out"][0][~on_box], moved_["out"][0][~on_box])
    # with motion a box pixel's taps are fractional: the box moved by no whole number of pixels
    assert any(len(t) >= 2 for (y, x), t in moved_["taps"].items() if on_box[y, x])


# ---- the input rules --------------------------------------------------------------------------------
def test_params_rule():
    ok = dict(normal_cos=0.9, plane_eps=0.1, max_len=8)
    assert T.check_params(**ok) is None
    for kw in (dict(normal_cos=-1.0), dict(normal_cos=1.0), dict(plane_eps=0.0), dict(max_len=1), dict(max_len=1024)):
        assert T.check_params(**{**ok, **kw}) is None, kw
    for kw in (dict(normal_cos=1.5), dict(normal_cos=-1.25), dict(normal_cos=float("nan")), dict(normal_cos=float("inf")),
               dict(plane_eps=float("nan")), dict(plane_eps=-1.0), dict(plane_eps=-0.0), dict(plane_eps=float("inf")),
               dict(max_len=0), dict(max_len=1025)):
        assert T.check_params(**{**ok, **kw}) is not None, kw


def test_camera_rule():
    """tan_half finite and > 0, vectors and position finite.  zoom 180: tanf of the float32
    pi / 2 is negative (-2.3e7), so the value decides, not the angle."""
    assert T.check_camera(TI.cam_a()) is None and T.check_camera(TI.cam_b()) is None
    for zoom in (1.0, 45.0, 90.0, 179.0):
        c = TI.cam_a().to_ctypes()
        c.zoom_deg = zoom
        assert T.check_camera(c) is None, zoom
    for name, c in TI.bad_cameras():
        assert T.check_camera(c) is not None, (name, T.camera_constants(c, 4, 3)["tan_half"])
