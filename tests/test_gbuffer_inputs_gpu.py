"""The two HIP G-buffer passes (k_raycast; k_bin_rect, k_bin_scan, k_bin_fill, k_bin_raster) on
the hostile catalogue of tests/gbuffer_inputs.py, bit for bit (vct_spec.h "G-buffer input
rule"): the caster against the CPU backend's restatement, the binned pass against the caster,
the binned pass twice on one context, and the rule's errors against the CPU backend's statuses.
tests/test_gbuffer_inputs.py checks the references themselves on the CPU."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_inputs as GI

pytestmark = pytest.mark.gpu
F = np.float32
CASES = {c.name: c for c in GI.legal_cases()}
ILLEGAL = GI.illegal_cases()
PLANES = ("pos", "nrm", "alb")
_want = {}


@pytest.fixture(scope="module")
def cpu_lib(oracle_mod):
    from vct import _lib
    return _lib.bind(C.CDLL(oracle_mod.CPU_BACKEND))


def _ctx(case, lib=None):
    from vct import Context
    v, i, m, k, mm = case.mesh.arrays()
    ctx = Context(GI.N, GI.G0, GI.E, lib=lib)
    if case.textures:
        ctx.set_textures(case.textures)
    ctx.voxelize(v, i, m, k, material_map=mm)
    return ctx


def _cpu_planes(cpu_lib, case):
    """The CPU backend's three planes of a case, computed once and left unchanged."""
    if case.name not in _want:
        ctx = _ctx(case, cpu_lib)
        bufs = [np.full((case.h, case.w, 4), 7.0, F) for _ in range(3)]
        ctx.gbuffer_raycast_device(case.cam, case.w, case.h, GI.ROUGH, *[b.ctypes.data for b in bufs])
        ctx.close()
        for b in bufs:
            b.setflags(write=False)
        _want[case.name] = bufs
    return _want[case.name]


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _diff(a, b):
    d = (a != b).any(-1)
    return f"{int(d.sum())} pixels differ, first (y, x) {np.argwhere(d)[:3].tolist()}"


@pytest.mark.parametrize("name", list(CASES))
def test_passes_equal_cpu_backend_and_each_other(gpu_ready, cpu_lib, name):
    """Raycast == CPU backend and raster == raycast on all three planes, bit for bit, with the
    outputs pre-filled (7.0 / -7.0); the raster call again on the same context (scratch reuse,
    the fill cursor that k_bin_scan resets) gives the same planes."""
    import torch
    case = CASES[name]
    want = [b.view(np.uint32) for b in _cpu_planes(cpu_lib, case)]
    ctx = _ctx(case)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dev = torch.device("cuda")
    ray = [torch.full((case.h, case.w, 4), 7.0, device=dev) for _ in range(3)]
    ras = [torch.full((case.h, case.w, 4), -7.0, device=dev) for _ in range(3)]
    again = [torch.full((case.h, case.w, 4), -7.0, device=dev) for _ in range(3)]
    ctx.gbuffer_raycast_device(case.cam, case.w, case.h, GI.ROUGH, *ray)
    ctx.gbuffer_raster_device(case.cam, case.w, case.h, GI.ROUGH, *ras)
    ctx.gbuffer_raster_device(case.cam, case.w, case.h, GI.ROUGH, *again)
    torch.cuda.synchronize()
    ctx.close()
    for plane, w_, a, b, c in zip(PLANES, want, ray, ras, again):
        a, b, c = _bits(a), _bits(b), _bits(c)
        assert np.array_equal(a, w_), f"{name} {plane}: raycast vs the CPU backend: {_diff(a, w_)}"
        assert np.array_equal(b, a), f"{name} {plane}: raster vs raycast: {_diff(b, a)}"
        assert np.array_equal(c, b), f"{name} {plane}: the second raster call: {_diff(c, b)}"
    assert int((want[0][..., 3] != 0).sum()) >= case.min_hits


def test_raster_across_frames_on_one_context(gpu_ready, cpu_lib):
    """One context through frames of different sizes and cameras, large to small and back: the
    binned pass's scratch (rectangles, counts, offsets, bins) carries nothing over."""
    import torch
    from vct import Context
    st = CASES["frame_520x500"]
    ctx = _ctx(st)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    dev = torch.device("cuda")
    order = ["frame_520x500", "frame_1x1", "frame_67x45_inside", "frame_16384x2", "frame_17x1", "frame_520x500"]
    for name in order:
        case = CASES[name]
        assert case.mesh is st.mesh
        out = [torch.full((case.h, case.w, 4), -7.0, device=dev) for _ in range(3)]
        ctx.gbuffer_raster_device(case.cam, case.w, case.h, GI.ROUGH, *out)
        torch.cuda.synchronize()
        for plane, w_, a in zip(PLANES, _cpu_planes(cpu_lib, case), out):
            assert np.array_equal(_bits(a), w_.view(np.uint32)), f"{name} {plane}"
    ctx.close()


@pytest.fixture(scope="module")
def both(gpu_ready, cpu_lib):
    case = CASES["near_eq_far"]
    hip, cpu = _ctx(case), _ctx(case, cpu_lib)
    yield hip, cpu
    hip.close()
    cpu.close()


@pytest.mark.parametrize("name", [c[0] for c in ILLEGAL])
def test_illegal_camera_status_and_untouched_buffers(both, name):
    """Every illegal camera of the rule: the CPU backend's status (VCT_EINVAL) from both passes,
    nothing written; afterwards the context renders a legal frame."""
    import torch
    from vct import VctError
    hip, cpu = both
    _, cam, w, h = next(c for c in ILLEGAL if c[0] == name)
    px = max(w, 1) * max(h, 1)
    dev = torch.device("cuda")
    for fn, fill in (("gbuffer_raycast_device", 7.0), ("gbuffer_raster_device", -7.0)):
        host = [np.full((px, 4), fill, F) for _ in range(3)]
        with pytest.raises(VctError) as want:
            getattr(cpu, fn)(cam, w, h, GI.ROUGH, *[b.ctypes.data for b in host])
        bufs = [torch.full((px, 4), fill, device=dev) for _ in range(3)]
        with pytest.raises(VctError) as got:
            # raw device pointers: the binding's own size check is not what is under test
            getattr(hip, fn)(cam, w, h, GI.ROUGH, *[b.data_ptr() for b in bufs])
        torch.cuda.synchronize()
        assert got.value.status == want.value.status == 1
        assert all(bool((b == fill).all()) for b in bufs) and all((b == F(fill)).all() for b in host)
    ok = [torch.zeros((16, 24, 4), device=dev) for _ in range(3)]
    hip.gbuffer_raster_device(GI.look(), 24, 16, GI.ROUGH, *ok)
    torch.cuda.synchronize()
    assert bool((ok[0][..., 3] != 0).all())
