"""vct_cone_query_device on the GPU against tests/query_ref.py (a numpy restatement of
vct_spec.h "cone queries", pinned to the CPU oracle's K4 and to spec_ref.Tracer.march in
tests/test_query.py).  Every comparison is bit-exact: the kernel runs the spec's float
operations in the spec's order, every cone is one lane's own, and the only atomic is the integer
step counter.  Grids are the Cornell box of lights_ref.cornell with light set S.  The kernel has
one address path (64-bit addresses), so there is no second path to force.
"""
import ctypes as C

import numpy as np
import pytest

import lights_ref
import query_ref as Q
import shadow_ref
import sky_view_ref as SV
from lights_ref import bits_equal
from test_query import EYE, shared_list, shared_reference, tau_min_frame

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 5
F = np.float32
NAN = float("nan")


def _ctx(n, lit=True, **kw):
    import torch
    from vct import Context
    ref = lights_ref.cornell(n)
    ctx = Context(n, ref["g0"], ref["E"], **kw)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.voxelize(*ref["arrays"])
    if lit:
        ctx.inject_lights(ref["lights"])
        ctx.build_mips()
    return ctx


def _query(ctx, cones):
    """-> (out4 [R, 4], steps [R], counter) of one call, the outputs pre-filled with NaN / -1."""
    import torch
    cones = np.array(cones, F).reshape(-1, 12)                 # a writable copy
    R = cones.shape[0]
    dev = torch.from_numpy(cones).cuda()
    out = torch.full((R, 4), NAN, device="cuda")
    steps = torch.full((R,), -1, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.cone_query_device(dev, R, out, steps, cnt)
    torch.cuda.synchronize()
    return out.cpu().numpy(), steps.cpu().numpy().astype(np.int64), int(cnt.item())


def _parity(n, cones, aniso=True, ref=None):
    c = lights_ref.cornell(n)
    if ref is None:
        ref = Q.march(Q.cornell_pyramid(n, aniso), n, aniso, c["g0"], c["E"], cones)
    ctx = _ctx(n, aniso=aniso)
    out, steps, total = _query(ctx, cones)
    ctx.close()
    bad = np.flatnonzero((out.view(np.uint32) != ref["out4"].view(np.uint32)).any(-1))
    assert not bad.size, f"{bad.size} cones differ, first {bad[:8]}: {out[bad[:2]]} != {ref['out4'][bad[:2]]}"
    assert np.array_equal(steps, ref["steps"])
    assert total == int(ref["steps"].sum())
    return ref


def _world(n, q):
    c = lights_ref.cornell(n)
    return np.array(c["g0"], F) + np.array(q, F) * (F(c["E"]) / F(n))


def test_one_cone(gpu_ready, oracle_mod):
    n = 4
    ref = _parity(n, Q.make_cones(_world(n, (2.0, 2.5, 3.0)), (0.3, -0.5, -1.0), 0.3))
    assert ref["steps"][0] > 0


def test_a_wave_and_one_lane(gpu_ready, oracle_mod):
    """n = 8, 65 cones: the diffuse cones of the first valid pixels of the 13 x 7 frame."""
    from test_shadow import gbuffer
    n = 8
    c = lights_ref.cornell(n)
    pos, nrm, _ = gbuffer(n)
    cones = Q.diffuse_cones(n, c["g0"], c["E"], pos, nrm, 9)[0]
    cones = cones[cones[:, 11] != 0][:65]
    assert cones.shape[0] == 65
    ref = _parity(n, cones)
    assert ref["steps"][64] > 0


@pytest.mark.parametrize("aniso", [True, False])
def test_shared_list(gpu_ready, oracle_mod, aniso):
    """The list tests/test_query.py pins and whose coverage it asserts: both identities, the
    hostile cones and the limited cones, more than 200 waves, six apertures inside a wave."""
    cones, _ = shared_list(16)
    _parity(16, cones, aniso, shared_reference(16, aniso))


def test_long_marches(gpu_ready, oracle_mod):
    """n = 64, the 48 x 36 frame at VCT_SPEC_TAU_MIN: marches past 64 steps."""
    n = 64
    c = lights_ref.cornell(n)
    ref = _parity(n, Q.specular_cones(n, c["g0"], c["E"], *tau_min_frame(n), EYE))
    assert int(ref["steps"].max()) >= 65


def test_hostile_cones(gpu_ready, oracle_mod):
    """The sixteen hand-written cones alone (less than a wave): non-finite records march nothing,
    and a skipped cone's out4 is overwritten with +0 and its steps with 0."""
    n = 16
    c = lights_ref.cornell(n)
    cones = Q.hostile_cones(n, c["g0"], c["E"])
    ctx = _ctx(n)
    out, steps, total = _query(ctx, cones)
    ctx.close()
    ref = Q.march(Q.cornell_pyramid(n), n, True, c["g0"], c["E"], cones)
    assert bits_equal(out, ref["out4"]) and np.array_equal(steps, ref["steps"]) and total == int(ref["steps"].sum())
    assert not out[[14, 15]].view(np.uint32).any() and not steps[[10, 11, 12, 13, 14, 15]].any()
    assert np.isfinite(out).all() and total > 0


def _gpu_frame(ctx, n):
    import torch
    from vct.camera import Camera
    w, h = shadow_ref.FRAMES[n]
    gb = [torch.empty((h, w, 4), device="cuda") for _ in range(3)]
    ctx.gbuffer_raycast_device(Camera(position=EYE), w, h, 0.1, *gb)
    torch.cuda.synchronize()
    gb[2] = torch.from_numpy(SV.pixel_roughness(gb[2].cpu().numpy())).cuda()
    return gb, w, h


def test_specular_identity_against_k4(gpu_ready, oracle_mod):
    """On the GPU's own frame: the specular-identity cones give vct_trace_device's spec4 and the
    steps of vct_trace_cones_device(VCT_CONES_SPECULAR)."""
    import torch
    from vct import VCT_CONES_SPECULAR
    n = 16
    c = lights_ref.cornell(n)
    ctx = _ctx(n)
    gb, w, h = _gpu_frame(ctx, n)
    D, S = torch.empty((h, w, 4), device="cuda"), torch.empty((h, w, 4), device="cuda")
    ctx.trace_device(*gb, w, h, EYE, D, S)
    S2 = torch.empty((h, w, 4), device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.trace_cones_device(VCT_CONES_SPECULAR, *gb, w, h, EYE, None, S2, cone_steps=cnt)
    torch.cuda.synchronize()
    pos, nrm, alb = (t.cpu().numpy() for t in gb)
    out, steps, total = _query(ctx, Q.specular_cones(n, c["g0"], c["E"], pos, nrm, alb, EYE))
    ctx.close()
    assert int((pos[..., 3] != 0).sum()) > 300
    assert bits_equal(out.reshape(h, w, 4), S.cpu().numpy())
    assert total == int(cnt.item()) > 0 and int(steps.sum()) == total


@pytest.mark.parametrize("n_diffuse", [9, 16])
def test_diffuse_identity_against_k4(gpu_ready, oracle_mod, n_diffuse):
    import torch
    from vct import VCT_CONES_DIFFUSE
    n = 16
    c = lights_ref.cornell(n)
    ctx = _ctx(n, n_diffuse=n_diffuse)
    gb, w, h = _gpu_frame(ctx, n)
    D = torch.empty((h, w, 4), device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.trace_cones_device(VCT_CONES_DIFFUSE, *gb, w, h, EYE, D, None, cone_steps=cnt)
    torch.cuda.synchronize()
    pos, nrm, _ = (t.cpu().numpy() for t in gb)
    cones, rows = Q.diffuse_cones(n, c["g0"], c["E"], pos, nrm, n_diffuse)
    out, _, total = _query(ctx, cones)
    ctx.close()
    got = Q.accumulate_diffuse(out, rows).reshape(h, w, 4)
    valid = pos[..., 3] != 0
    assert bits_equal(got[valid], D.cpu().numpy()[valid])
    assert total == int(cnt.item()) > 0


def test_a_permuted_list_gives_the_permuted_outputs(gpu_ready, oracle_mod):
    """No lane depends on another lane's cone: the n = 16 list under a fixed random permutation."""
    cones, _ = shared_list(16)
    ref = shared_reference(16)
    perm = np.random.default_rng(20).permutation(cones.shape[0])
    ctx = _ctx(16)
    out, steps, total = _query(ctx, cones[perm])
    ctx.close()
    assert bits_equal(out, ref["out4"][perm]) and np.array_equal(steps, ref["steps"][perm])
    assert total == int(ref["steps"].sum())


def test_optional_outputs_may_be_null(gpu_ready, oracle_mod):
    import torch
    cones, parts = shared_list(16)
    part = np.array(cones[parts["spec block"]])
    ref = shared_reference(16)["out4"][parts["spec block"]]
    ctx = _ctx(16)
    out = torch.full((part.shape[0], 4), NAN, device="cuda")
    ctx.cone_query_device(torch.from_numpy(part).cuda(), part.shape[0], out)
    torch.cuda.synchronize()
    ctx.close()
    assert bits_equal(out.cpu().numpy(), ref)


def test_errors(gpu_ready, oracle_mod):
    """Through the C-ABI: count = 0 is VCT_OK, NULL or misaligned pointers are VCT_EINVAL, and
    VCT_ESTATE before the mips; none of them writes anything."""
    import torch
    from vct import _lib
    n = 8
    lib = _lib.load()
    fn = _lib.bind_query_extension(lib, "vct_cone_query_device")
    c = lights_ref.cornell(n)
    ctx = _ctx(n, lit=False)
    R = 8
    cones = torch.from_numpy(np.tile(Q.make_cones(_world(n, (4.0, 4.0, 4.0)), (0.0, 0.0, -1.0), 0.3), (R + 1, 1))).cuda()
    out = torch.full((R + 1, 4), 5.0, device="cuda")
    steps = torch.full((R + 1,), 6, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    p, o, s, k = (t.data_ptr() for t in (cones, out, steps, cnt))

    def call(cones=p, count=R, out4=o, st=s, total=k, args=True):
        a = _lib.VctConeQueryArgs()
        a.cones, a.count, a.out4, a.steps, a.cone_steps = cones, count, out4, st, total
        return fn(ctx.h, C.byref(a) if args else None)

    assert call() == ESTATE                                               # voxelized, no level 0
    ctx.inject_lights(c["lights"])
    assert call() == ESTATE                                               # no mips
    ctx.build_mips()
    cases = {
        "NULL args": dict(args=False), "NULL cones": dict(cones=None), "NULL out4": dict(out4=None),
        "misaligned cones": dict(cones=p + 4), "misaligned cones by 8": dict(cones=p + 8),
        "misaligned out4": dict(out4=o + 4), "misaligned steps": dict(st=s + 2),
        "misaligned cone_steps": dict(total=k + 4),
    }
    for what, kw in cases.items():
        assert call(**kw) == EINVAL, what
        assert lib.vct_last_error(ctx.h), what
    assert call(count=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((steps == 6).all()) and not bool(cnt.any())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[:R] != 5.0).any()) and bool((out[R] == 5.0).all()) and int(steps[R]) == 6
    assert int(cnt[0]) == int(steps[:R].sum()) > 0 and int(cnt[1]) == 0
    ctx.close()
