"""The consumers that start the hard voxel walk from a caller's pixel, on the hostile-receiver
catalogue (tests/receiver_inputs.py), against the references that tests/test_receiver_inputs.py
holds to the hand-written V: vct_composite_device (the oracle), vct_composite_lights_device and
vct_composite_emissive_device with vis NULL (lights_ref), vct_shadow_cones_device and
vct_composite_shadowed_device (shadow_ref).  n = 16, frames of at most 64 x 24, every float
output compared through a uint32 view, cone_steps equal; RGBA8 within 1, the composite tests'
bar for the device powf.

Only the "slabs" field runs here.  On it a NaN component converted to cell 0 lands in an
occupied cell, so a kernel that started a walk without the "shadow-walk receiver rule" of
include/vct_spec.h would return 0 from the walk's first cell and fail these tests by value; on
the "open" field the same mistake could be a walk that never ends, which is why that field
stays with the CPU references (bounded there by their cell count).

Also here: the context's alpha step-table set (vct_shadow.hip step_tables), driven past its 64
apertures so that it starts again, alone and alternating two streams."""
import numpy as np
import pytest

import light_inputs as LI
import lights_ref
import receiver_inputs as RI
import shadow_ref
import sky_ref

pytestmark = pytest.mark.gpu
F = np.float32
N = RI.N_GRID
EINVAL = 1
MIXED = [0.0, 0.1, 0.05, 0.0, 0.3, 0.0, 0.02, 0.2]       # hard and soft lights inside one call
KE = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [2.0, 1.0, 0.5, 0.0]], F)   # material 3 emits

_cpu = {}


def _refs(O):
    """What every test shares, computed once on the CPU and left unchanged: the field through the
    oracle's K1, the frames, the light list, the alpha pyramid and the shadow_ref planes."""
    if not _cpu:
        cat = RI.catalogue()
        f = RI.field("slabs")
        ao, nm = LI.voxels(O, f)
        RI.check_field("slabs", ao)
        l0 = np.zeros_like(ao)
        l0[..., 3] = (ao[..., 3] != 0).astype(F)
        _cpu.update(cat=cat, f=f, ao=ao, nm=nm, occ=ao[..., 3] != 0, comp=RI.build(f, ao, nm, cat),
                    planes=RI.build(f, ao, nm, cat, composite=False), clean=RI.build(f, ao, nm, []),
                    lights=RI.light_list(), alpha=shadow_ref.alpha_pyramid(N, l0, True), shadow={})
        for a in (ao, nm, *_cpu["comp"][:5], *_cpu["planes"][:5]):
            a.setflags(write=False)
    return _cpu


def _tan(kind, n):
    return {"hard": [0.0] * n, "soft": [0.1] * n, "mixed": (MIXED * 8)[:n]}[kind]


def _shadow_ref(c, key, pos, nrm, kind):
    if (key, kind) not in c["shadow"]:
        c["shadow"][(key, kind)] = shadow_ref.shadow(N, RI.G0, RI.E, c["ao"], c["alpha"], True, pos, nrm, c["lights"],
                                                     _tan(kind, len(c["lights"])))
    return c["shadow"][(key, kind)]


def _ctx(c, emit=False):
    import torch
    from vct import Context
    f = c["f"]
    ctx = Context(N, f.g0, f.E)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.voxelize(f.verts, f.idx, f.mat, f.kd)
    if emit:
        ctx.voxelize_emission(f.verts, f.idx, f.mat, KE)
    ctx.inject_lights(c["lights"])
    ctx.build_mips()
    ao, _ = ctx.download_voxels()
    assert np.array_equal(RI.bits(ao), RI.bits(c["ao"])), "K1 on the GPU is the oracle's field"
    assert np.array_equal(ctx.download_level(0)[..., 3] != 0, c["occ"])
    return ctx


def _dev(fr):
    import torch
    return [torch.from_numpy(np.array(a, F)).cuda() for a in (fr.pos, fr.nrm, fr.alb, fr.D, fr.S)]


def _same(got, want, fr, what):
    d = (RI.bits(got) != RI.bits(want)).reshape(fr.entry.shape + (-1,)).any(-1)
    assert not d.any(), f"{what}: {int(d.sum())} pixels differ, first: {RI.describe(fr, d)}"


def _rgba_within_1(got, want, what):
    got, want = np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32)
    for sh in (0, 8, 16, 24):
        assert np.abs(((got >> sh) & 255).astype(np.int64) - ((want >> sh) & 255).astype(np.int64)).max() <= 1, what


def _cones(ctx, pos, nrm, lights, tan):
    import torch
    h, w = pos.shape[:2]
    vis = torch.full((len(lights), h, w), float("nan"), device="cuda")
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.shadow_cones_device(pos, nrm, w, h, lights, tan, vis, steps)
    torch.cuda.synchronize()
    return vis, vis.cpu().numpy(), int(steps.item())


def test_composite_device(gpu_ready, oracle_mod):
    """vct_composite_device: every entry x every directional light against the oracle (which
    equals the hand-written V, checked again here): the linear frame bit for bit, RGBA8 within 1."""
    import torch
    c = _refs(oracle_mod)
    fr = c["comp"]
    h, w = fr.entry.shape
    ctx = _ctx(c)
    gb = _dev(fr)
    lin = torch.empty((h, w, 4), device="cuda")
    rgba = torch.empty((h, w), dtype=torch.int32, device="cuda")
    for e in RI.directions():
        want, want_rgba = oracle_mod.composite(N, RI.G0, RI.E, c["ao"], fr.pos, fr.nrm, fr.alb, fr.D, fr.S, e.d, RI.COLOUR)
        V = RI.expected_v(fr, c["cat"], c["occ"], e.d)
        assert np.array_equal(RI.bits(want), RI.bits(RI.composite_expect(fr, e.d, RI.COLOUR, V))), e.name
        lin.fill_(float("nan"))
        ctx.composite_device(*gb, w, h, e.d, RI.COLOUR, out_linear4=lin, out_rgba8=rgba)
        torch.cuda.synchronize()
        _same(lin.cpu().numpy(), want, fr, f"composite, light {e.name}")
        _rgba_within_1(rgba.cpu().numpy(), want_rgba, e.name)
    ctx.close()


def test_composite_lights_and_emissive(gpu_ready, oracle_mod):
    """vct_composite_lights_device with the whole list (20 directional lights, a point and a spot
    light) and every light alone, and vct_composite_emissive_device with vis NULL at scale 0 and
    1.5 over a live emission grid (Em = +0 on every NaN or far-out pixel: the lookup tests the
    floats first), against lights_ref and emission_ref."""
    import torch
    import emission_ref
    c = _refs(oracle_mod)
    fr, lights = c["comp"], c["lights"]
    h, w = fr.entry.shape
    ctx = _ctx(c, emit=True)
    assert ctx.emission_voxels() > 0
    gb = _dev(fr)
    lin = torch.empty((h, w, 4), device="cuda")
    rgba = torch.empty((h, w), dtype=torch.int32, device="cuda")
    want = lights_ref.composite(N, RI.G0, RI.E, c["ao"], fr.pos, fr.nrm, fr.alb, fr.D, fr.S, lights)
    assert np.isfinite(want).all()
    ctx.composite_lights_device(*gb, w, h, lights, out_linear4=lin, out_rgba8=rgba)
    torch.cuda.synchronize()
    _same(lin.cpu().numpy(), want, fr, "composite_lights, the list")
    px = rgba.cpu().numpy()
    for j, light in enumerate(lights):
        one = lights_ref.composite(N, RI.G0, RI.E, c["ao"], fr.pos, fr.nrm, fr.alb, fr.D, fr.S, [light])
        ctx.composite_lights_device(*gb, w, h, [light], out_linear4=lin)
        torch.cuda.synchronize()
        _same(lin.cpu().numpy(), one, fr, f"composite_lights, light {j} alone")
    Em, hit = emission_ref.lookup(N, RI.G0, RI.E, ctx.download_emission(), fr.pos)
    # Em = +0 on every NaN or far-out pixel; an edge entry whose P lies in cell 0 of the emitting slab has its E
    assert hit.sum() > 50 and all(c["cat"][i].family == "edge" for i in fr.entry[hit & (fr.entry >= 0)])
    for scale in (0.0, 1.5):
        lin.fill_(float("nan"))
        ctx.composite_emissive_device(*gb, w, h, lights, None, scale, out_linear4=lin, out_rgba8=rgba)
        torch.cuda.synchronize()
        _same(lin.cpu().numpy(), emission_ref.composite(want, fr.pos, Em, scale), fr, f"composite_emissive, scale {scale}")
        if scale == 0.0:
            assert np.array_equal(rgba.cpu().numpy(), px)
    ctx.close()


def _check_planes(c, ctx, key, pos, nrm, kind, entries=None, fr=None):
    """One vct_shadow_cones_device call against shadow_ref; -> (vis tensor, planes, reference)."""
    import torch
    lights = c["lights"]
    ref = _shadow_ref(c, key, pos, nrm, kind)
    vis, got, steps = _cones(ctx, torch.from_numpy(np.array(pos, F)).cuda(),
                             torch.from_numpy(np.array(nrm, F)).cuda(), lights, _tan(kind, len(lights)))
    for j in range(len(lights)):
        d = RI.bits(got[j]) != RI.bits(ref["vis"][j])
        where = RI.describe(fr, d) if fr is not None else np.argwhere(d)[:8].tolist()
        assert not d.any(), f"{key} {kind}: plane {j}: {int(d.sum())} pixels differ, first: {where}"
    assert steps == ref["steps"], (key, kind, steps, ref["steps"])
    return vis, got, ref


def test_shadow_cones(gpu_ready, oracle_mod):
    """vct_shadow_cones_device on every entry, the (+inf) + (-inf) family included: the list
    once all hard, once all soft, once mixed inside one call, on the full frame, on a partial
    13 x 7 frame and on an 8 x 8 block of NaN pixels with one normal (the lights that normal
    faces away from are skipped on the wave's ballot).  Planes and cone_steps equal shadow_ref;
    a NaN receiver's hard V equals its soft V (1 where the light is not skipped)."""
    c = _refs(oracle_mod)
    fr = c["planes"]
    ctx = _ctx(c)
    got = {}
    for kind in ("hard", "soft", "mixed"):
        _, got[kind], ref = _check_planes(c, ctx, "full", fr.pos, fr.nrm, kind, fr=fr)
    nanq = np.isnan(RI.origin(fr.pos, fr.nrm)).any(-1) & (fr.pos[..., 3] != 0)
    assert nanq.sum() == 136
    assert np.array_equal(RI.bits(got["hard"][:, nanq]), RI.bits(got["soft"][:, nanq]))
    assert set(np.unique(got["hard"][:, nanq]).tolist()) == {0.0, 1.0}
    assert (got["hard"][:20, nanq] == 1).any(0).all(), "every NaN receiver is lit by some directional light"
    assert not got["hard"][20:, nanq].any(), "the point and the spot light skip a NaN receiver (r2 > 0)"
    for name, pos, nrm, ents in RI.small_frames(c["cat"]):
        for kind in ("hard", "soft", "mixed"):
            _, g, ref = _check_planes(c, ctx, name, pos, nrm, kind)
            if name.startswith("NaN block"):
                assert ref["steps"] == 0
                lit = [j for j in range(20) if RI.ndl_of(ents[0].N, RI.directions()[j].d) > 0]
                assert 0 < len(lit) < 20
                assert all((g[j] == (1.0 if j in lit else 0.0)).all() for j in range(len(c["lights"])))
    ctx.close()


def test_shadow_cones_64_bit_path(gpu_ready, oracle_mod):
    """The hard-path cases again under vct_debug_shadow(1), the 64-bit address path."""
    from vct import _lib
    c = _refs(oracle_mod)
    fr = c["planes"]
    ctx = _ctx(c)
    lib = _lib.load()
    _lib.debug_shadow(lib, True)
    try:
        for kind in ("hard", "mixed"):
            _check_planes(c, ctx, "full", fr.pos, fr.nrm, kind, fr=fr)
            assert _lib.debug_shadow_path(ctx.lib, ctx.h) == 64
        for name, pos, nrm, _ in RI.small_frames(c["cat"]):
            _check_planes(c, ctx, name, pos, nrm, "mixed")
    finally:
        _lib.debug_shadow(lib, False)
    ctx.close()


def test_composite_shadowed_and_the_clean_frame_afterwards(gpu_ready, oracle_mod):
    """vct_composite_shadowed_device over the mixed planes of the composite frame against
    shadow_ref.composite; and a clean frame (the field's own pixels) gives the same planes and
    the same composite after the hostile frame as before it."""
    import torch
    c = _refs(oracle_mod)
    fr, clean, lights = c["comp"], c["clean"], c["lights"]
    ctx = _ctx(c)
    h, w = clean.entry.shape
    cgb = _dev(clean)
    d0 = RI.directions()[-2].d

    def clean_pass():
        _, planes, steps = _cones(ctx, cgb[0], cgb[1], lights, _tan("mixed", len(lights)))
        lin = torch.empty((h, w, 4), device="cuda")
        ctx.composite_device(*cgb, w, h, d0, RI.COLOUR, out_linear4=lin)
        torch.cuda.synchronize()
        return planes, steps, lin.cpu().numpy()

    before = clean_pass()
    ref = _shadow_ref(c, "clean", clean.pos, clean.nrm, "mixed")
    assert np.array_equal(RI.bits(before[0]), RI.bits(ref["vis"])) and before[1] == ref["steps"] and ref["steps"] > 0
    vis, _, ref = _check_planes(c, ctx, "comp", fr.pos, fr.nrm, "mixed", fr=fr)
    hh, ww = fr.entry.shape
    gb = _dev(fr)
    lin = torch.full((hh, ww, 4), float("nan"), device="cuda")
    rgba = torch.empty((hh, ww), dtype=torch.int32, device="cuda")
    ctx.composite_shadowed_device(*gb, ww, hh, lights, vis, out_linear4=lin, out_rgba8=rgba)
    torch.cuda.synchronize()
    want = shadow_ref.composite(N, RI.G0, RI.E, fr.pos, fr.nrm, fr.alb, fr.D, fr.S, lights, ref["vis"])
    assert np.isfinite(want).all()
    _same(lin.cpu().numpy(), want, fr, "composite_shadowed")
    after = clean_pass()
    assert np.array_equal(RI.bits(after[0]), RI.bits(before[0])) and after[1] == before[1]
    assert np.array_equal(RI.bits(after[2]), RI.bits(before[2]))
    ctx.close()


# ---------------------------------------------------------------------------
# the context's alpha step-table set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("streams", [1, 2])
def test_step_table_set_starts_again(gpu_ready, oracle_mod, streams):
    """step_tables keeps at most 64 apertures per context and starts the set again when a new
    one does not fit.  n = 8, a 13 x 7 frame: three calls of 30 distinct apertures each (the
    third does not fit), a vct_sky_cones_device call (it shares the set), the first call again,
    the second again (the set starts again once more); every plane equals shadow_ref / sky_ref
    bit for bit, and the steps.  streams = 2: the calls alternate between two streams, the
    first behind other work, as test_first_use_on_one_stream_second_on_another queues them.
    An aperture list that needs more than 64 tables in one call cannot be passed:
    VCT_MAX_LIGHTS is 64, and the 65-light refusal comes first and leaves the set as it was."""
    import torch
    from test_shadow_gpu import _ctx as cornell_ctx, _gbuffer
    from vct import VctError
    n = 8
    ref0 = lights_ref.cornell(n)
    ctx = cornell_ctx(n)
    gb = _gbuffer(ctx, n)
    h, w = gb[0].shape[:2]
    assert (w, h) == (13, 7)
    pos, nrm = gb[0].cpu().numpy(), gb[1].cpu().numpy()
    lights = (shadow_ref.lights_for(n) * 4)[:30]
    tans = [[float(F(base + 0.01 * i)) for i in range(30)] for base in (0.02, 0.32, 0.62)]
    assert len({shadow_ref.clamp_tau(t) for ts in tans for t in ts}) == 90
    want = [shadow_ref.reference(n, pos, nrm, lights=lights, tan_half=ts) for ts in tans]
    want_sky = sky_ref.frame(n, ref0["g0"], ref0["E"], shadow_ref.cornell_alpha(n), True, pos, nrm, sky_ref.SKY_TILTED, 9)
    order = [0, 1, 2, "sky", 0, 1]
    qs = [torch.cuda.Stream() for _ in range(streams)] if streams > 1 else [torch.cuda.current_stream()]
    if streams > 1:
        busy = torch.rand((2048, 2048), device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(qs[0]):
            for _ in range(8):                                   # the first stream is busy when the first call is queued
                busy = busy @ busy * 1e-3
    outs, steps = [], torch.zeros(len(order), dtype=torch.int64, device="cuda")
    for k, what in enumerate(order):
        ctx.set_stream(qs[k % len(qs)].cuda_stream)
        if what == "sky":
            out = torch.full((h, w, 4), float("nan"), device="cuda")
            ctx.sky_cones_device(gb[0], gb[1], w, h, sky_ref.to_ctypes(sky_ref.SKY_TILTED), out, None, steps[k:k + 1])
        else:
            out = torch.full((30, h, w), float("nan"), device="cuda")
            ctx.shadow_cones_device(gb[0], gb[1], w, h, lights, tans[what], out, steps[k:k + 1])
        outs.append(out)
    torch.cuda.synchronize()
    for k, what in enumerate(order):
        if what == "sky":
            assert lights_ref.bits_equal(outs[k].cpu().numpy(), want_sky["sky4"]), "the sky call on the restarted set"
            assert int(steps[k]) == want_sky["steps"]
        else:
            bad = [j for j in range(30) if not lights_ref.bits_equal(outs[k][j].cpu().numpy(), want[what]["vis"][j])]
            assert not bad, f"call {k} (aperture set {what}): planes {bad} differ"
            assert int(steps[k]) == want[what]["steps"] and want[what]["steps"] > 0
    # 65 lights, 65 distinct apertures: refused before the set is touched
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    vis = torch.full((65, h, w), 3.0, device="cuda")
    with pytest.raises(VctError) as e:
        ctx.shadow_cones_device(gb[0], gb[1], w, h, (lights * 3)[:65], [0.021 + 0.013 * i for i in range(65)], vis)
    assert e.value.status == EINVAL
    out = torch.full((30, h, w), float("nan"), device="cuda")
    ctx.shadow_cones_device(gb[0], gb[1], w, h, lights, tans[1], out)         # the set still serves its apertures
    torch.cuda.synchronize()
    assert bool((vis == 3.0).all())
    assert lights_ref.bits_equal(out.cpu().numpy(), want[1]["vis"])
    ctx.close()
