"""Light bounces without a GPU: the boundary declares and binds the two functions, a
library without them (the CPU oracle backend) still loads, and the reference the GPU tests
compare against (tests/bounce_ref.py) has the properties vct_spec.h "light bounces" states.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bounce_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref(oracle_mod):
    return bounce_ref.cornell(32, True, 9, 2)


def test_header_declares_bounce_functions():
    src = open(os.path.join(REPO, "include", "vct_bounce.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"vct_status\s+vct_inject_bounces\s*\(\s*vct_ctx\s*\*\s*\w*\s*,\s*uint32_t\s+\w+\s*\)\s*;", code)
    assert re.search(r"vct_status\s+vct_bounce_sources\s*\(\s*vct_ctx\s*\*\s*\w*\s*,\s*uint32_t\s*\*\s*\w+\s*\)\s*;",
                     code)
    vct_h = open(os.path.join(REPO, "include", "vct.h")).read()
    assert '#include "vct_bounce.h"' in vct_h                 # a host that includes vct.h sees them
    assert re.search(r"#define\s+VCT_ABI_VERSION\s+1\b", vct_h)   # additive: the version stays
    spec = open(os.path.join(REPO, "include", "vct_spec.h")).read()
    assert "light bounces" in spec


def test_binding_lists_them_and_hip_library_exports_them():
    import subprocess
    from vct import Context, _lib
    assert set(_lib.EXTENSIONS) == {"vct_inject_bounces", "vct_bounce_sources"}
    assert not set(_lib.EXTENSIONS) & set(_lib.EXPORTS)
    assert callable(Context.inject_bounces) and callable(Context.bounce_sources)
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vct_[a-z0-9_]+)", out))
    assert set(_lib.EXTENSIONS) <= exported
    for name in _lib.EXTENSIONS:
        fn = _lib.bind_extension(lib, name)
        assert fn.restype is C.c_int32 and fn.argtypes[0] is C.c_void_p
    assert _lib.bind_extension(lib, "vct_inject_bounces")(None, 1) == 1     # VCT_EINVAL, no device needed
    assert _lib.bind_extension(lib, "vct_bounce_sources")(None, None) == 1


def test_library_without_them_still_loads(oracle_mod):
    """The CPU backend exports vct.h only: it binds, runs, and refuses a bounce by name."""
    from helpers import scene_arrays
    from vct import Context, _lib, scenes
    cpu = _lib.bind(C.CDLL(oracle_mod.CPU_BACKEND))
    for name in _lib.EXTENSIONS:
        assert not hasattr(cpu, name)
        with pytest.raises(AttributeError, match=name):
            _lib.bind_extension(cpu, name)
    s, (v, i, m, k) = scene_arrays("cornell")
    g0, E = scenes.grid_for_unit_box(16)
    ctx = Context(16, g0, E, lib=cpu)
    ctx.voxelize(v, i, m, k)
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    ctx.build_mips()
    before = ctx.download_level(0)
    with pytest.raises(AttributeError, match="vct_inject_bounces"):
        ctx.inject_bounces(1)
    with pytest.raises(AttributeError, match="vct_bounce_sources"):
        ctx.bounce_sources()
    assert np.array_equal(ctx.download_level(0), before)
    ctx.close()


def test_reference_inputs(ref):
    """Cornell at 32^3: the figures the GPU tests rely on."""
    g = ref["grid"]
    (z, y, x), (zz, zy, zx) = bounce_ref.sources(g["albedo_occ"], g["normal"])
    assert int((g["counts"] > 0).sum()) == 5694
    assert zz.size == 99 and x.size == 5595 and x.size % 64 != 0
    b = ref["bounces"]
    assert b[1]["steps"] == 296410
    L0, L1 = b[0]["level0"], b[1]["level0"]
    changed = np.any(L0[z, y, x, :3] != L1[z, y, x, :3], axis=-1)
    print("bounce 1 changes", changed.sum(), "of", x.size, "sources")
    assert changed.sum() > x.size // 2          # an implementation that does nothing cannot pass
    black = ~np.any(L0[z, y, x, :3] != 0, axis=-1)
    lit = black & np.any(L1[z, y, x, :3] != 0, axis=-1)
    print("bounce 1 lights", lit.sum(), "voxels that direct light left black")
    assert lit.sum() == 4992


def test_reference_is_jacobi(ref, oracle_mod):
    """L2 = L0 + A * I(L1) bit for bit, with I(L1) gathered here from L1's own pyramid, and
    not L1 + A * I(L1) (Gauss-Seidel on the light: the direct light counted twice).
    The identity is asserted in the order it is computed in: read as a float subtraction,
    L2 - L0 == A * I(L1) rounds once more and differs in the last bit for 1 344 of the
    16 785 source channels here, for a reference that is exactly Jacobi."""
    g, b = ref["grid"], ref["bounces"]
    n, g0, E = 32, ref["g0"], ref["E"]
    gbuf, (z, y, x) = bounce_ref.source_gbuffer(n, g0, E, g["albedo_occ"], g["normal"])
    L0, L1, L2 = (b[k]["level0"] for k in range(3))
    I1, _ = bounce_ref.gather(oracle_mod, n, g0, E, L1, oracle_mod.build_mips(n, L1, True), gbuf, True, 9)
    A = g["albedo_occ"][z, y, x, :3]
    assert bounce_ref.bits_equal(L2[z, y, x, :3], L0[z, y, x, :3] + A * I1)
    assert not np.array_equal(L2[z, y, x, :3], L1[z, y, x, :3] + A * I1)
    assert not np.array_equal(L2, L1)                         # the second bounce sees the first
    for k in (1, 2):                                          # alpha is L0's
        assert bounce_ref.bits_equal(b[k]["level0"][..., 3], L0[..., 3])


def test_zero_normal_and_empty_voxels_keep_level0(ref):
    g, b = ref["grid"], ref["bounces"]
    _, (zz, zy, zx) = bounce_ref.sources(g["albedo_occ"], g["normal"])
    empty = g["albedo_occ"][..., 3] == 0
    for k in (1, 2):
        L = b[k]["level0"]
        assert bounce_ref.bits_equal(L[zz, zy, zx], b[0]["level0"][zz, zy, zx])
        assert not L[empty].view(np.uint32).any()             # +0, every channel


def test_zero_bounces_is_identity(ref, oracle_mod):
    g = ref["grid"]
    out = bounce_ref.bounce(oracle_mod, 32, ref["g0"], ref["E"], g["albedo_occ"], g["normal"], g["r0"], 0)
    assert len(out) == 1 and bounce_ref.bits_equal(out[0]["level0"], g["r0"])
    assert bounce_ref.bits_equal(out[0]["pyr"], g["pyr"])
    nd0 = bounce_ref.bounce(oracle_mod, 32, ref["g0"], ref["E"], g["albedo_occ"], g["normal"], g["r0"], 1,
                            n_diffuse=0)
    assert bounce_ref.bits_equal(nd0[1]["level0"], g["r0"])   # no cone: I = 0
