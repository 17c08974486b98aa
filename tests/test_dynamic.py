"""The dynamic layer without a GPU: the property its retraction stands on (the oracle's sums
and counts are additive over a concatenation), the catalogue of tests/dynamic_ref.py keeps what
its names promise, the boundary declares, binds and exports the three functions of
include/vct_dynamic.h, a library without them still loads, and the host refuses malformed
--dynamic flags.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dynamic_ref as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "voxel-based-global-illumination_amd", "build", "vct_headless")
NAMES = ("vct_voxelize_dynamic", "vct_voxelize_dynamic_device", "vct_dynamic_voxels")
SIZES = (16, 32, 64)          # the grids tests/test_dynamic_gpu.py uses


# ---- additivity: what makes an exact retraction possible ----------------------------------------
@pytest.mark.parametrize("n", D.GRIDS)
def test_sums_and_counts_are_additive(oracle_mod, n):
    """oracle(union(S, A)) = oracle(S) + oracle(A) elementwise, for every layer of the catalogue
    and the first positions of the path (integer sums: no rounding depends on the order)."""
    s_sums, s_cnt = D.static_coverage(n)
    named = [(k, v) for k, v in D.layers().items()] + [(f"path{i}", m) for i, m in enumerate(D.path()[:3])]
    for name, layer in named:
        a_sums, a_cnt = D.coverage(n, layer)
        u_sums, u_cnt = D.coverage(n, D.union(D.static_arrays(), layer))
        assert np.array_equal(u_cnt, s_cnt + a_cnt), name
        assert np.array_equal(u_sums, s_sums + a_sums), name


def test_union_offsets_indices_and_materials():
    sv, si, sm, sk = D.static_arrays()
    lv, li, lm, lk = D.layers()["tet"]
    v, i, m, k = D.union((sv, si, sm, sk), (lv, li, lm, lk))
    assert v.shape[0] == sv.shape[0] + lv.shape[0] and i.size == si.size + li.size
    assert np.array_equal(i[:si.size], si) and np.array_equal(i[si.size:], li + sv.shape[0])
    assert np.array_equal(m[sm.size:], lm + sk.shape[0]) and np.array_equal(k[sk.shape[0]:], lk)
    assert np.array_equal(v[i[si.size:]], lv[li])
    e = D.union((sv, si, sm, sk), D.layers()["empty"])
    assert np.array_equal(e[0], sv) and np.array_equal(e[1], si) and np.array_equal(e[2], sm)


# ---- the catalogue is not vacuous -----------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_catalogue_keeps_its_promises(oracle_mod, n):
    """Each layer's class, against the static occupancy: the overlapping layers hit voxels S
    occupies and voxels S leaves empty; `air` hits only empty voxels; `outside` and `empty` hit
    none (the no-candidate and no-triangle paths)."""
    S = D.static_coverage(n)[1] > 0
    hit = {k: D.layer_coverage(n, k)[1] > 0 for k in D.layers()}
    for k in ("floor", "tet", "over", "straddle"):
        assert (hit[k] & S).sum() >= 1 and (hit[k] & ~S).sum() >= 1, (n, k)
    assert hit["air"].sum() >= 8 and not (hit["air"] & S).any()
    assert not hit["outside"].any() and not hit["empty"].any()
    assert D.layers()["outside"][1].size == 36 and D.layers()["empty"][1].size == 0
    assert D.layers()["floor"][1].size == 36 and D.layers()["tet"][1].size == 12
    assert set(D.ADD) | set(D.REPLACE) <= set(hit)


@pytest.mark.parametrize("n", SIZES)
def test_replace_steps_vacate_occupy_and_share(oracle_mod, n):
    """floor -> tet -> over: each step vacates a voxel, newly occupies one, and has a voxel both
    layers hit (tet stands 0.02 beside floor: disjoint solids, shared voxels; over overlaps
    tet).  The last step, -> none, vacates only."""
    S = D.static_coverage(n)[1] > 0
    hit = [D.layer_coverage(n, k)[1] > 0 for k in D.REPLACE]
    assert D.REPLACE[-1] == "empty"
    for a, b in zip(hit[:-2], hit[1:-1]):
        before, after = S | a, S | b
        assert (before & ~after).sum() >= 1 and (after & ~before).sum() >= 1 and (a & b).sum() >= 1
    assert ((S | hit[-2]) & ~S).sum() >= 1


@pytest.mark.parametrize("n", D.GRIDS)
def test_path_re_enters_voxels(oracle_mod, n):
    """The moving box leaves voxels at every step and is back in some of them eight steps later."""
    S = D.static_coverage(n)[1] > 0
    hit = [D.coverage(n, m)[1] > 0 for m in D.path()]
    assert len(hit) == 24
    for i in range(23):
        left = hit[i] & ~hit[i + 1]
        assert left.any() and (hit[i + 1] & ~hit[i]).any(), i
        assert (hit[i] & ~S).any()
    for i in range(16):
        assert np.array_equal(hit[i], hit[i + 8])
        assert ((hit[i] & ~hit[i + 1]) & hit[i + 8]).any(), i


# ---- the boundary -----------------------------------------------------------------------------------
def test_header_and_spec_declare_the_functions():
    src = open(os.path.join(REPO, "include", "vct_dynamic.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(rf"vct_status\s+{name}\s*\(\s*vct_ctx\s*\*", code), name
    for text in ("VCT_ESTATE", "n_idx == 0", "vct_save_grid", "Kd materials only", "ties go to the lower index"):
        assert text in src, text
    vct_h = open(os.path.join(REPO, "include", "vct.h")).read()
    assert vct_h.count('#include "vct_dynamic.h"') == 1
    assert re.search(r"#define\s+VCT_ABI_VERSION\s+1\b", vct_h)
    assert not any(name in vct_h for name in NAMES)
    spec = open(os.path.join(REPO, "include", "vct_spec.h")).read()
    block = spec.split("---- dynamic layer", 1)[1]
    for text in ("union(S, D)", "modulo 2^64", "all-zero record", "K1 input rule", "2^31", "vct_load_grid"):
        assert text in block, text


def test_binding_lists_them_and_hip_library_exports_them():
    from vct import Context, _lib
    assert _lib.DYNAMIC_EXTENSIONS == NAMES
    assert not set(NAMES) & (set(_lib.EXPORTS) | set(_lib.EXTENSIONS) | set(_lib.LIGHT_EXTENSIONS) |
                             set(_lib.SHADOW_EXTENSIONS) | set(_lib.EMISSION_EXTENSIONS) | set(_lib.SKY_EXTENSIONS))
    assert len(_lib.EXPORTS) == 52                                            # vct.h's list is untouched
    for m in ("voxelize_dynamic", "voxelize_dynamic_device", "dynamic_voxels"):
        assert callable(getattr(Context, m)), m
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vct_[a-z0-9_]+)", out))
    assert set(NAMES) <= exported
    assert lib.vct_abi_version() == 1
    # VCT_EINVAL for a NULL ctx, no device needed
    n = C.c_uint32()
    assert _lib.bind_dynamic_extension(lib, "vct_voxelize_dynamic")(None, None, 12, 0, None, 0, None, None, 0) == 1
    assert _lib.bind_dynamic_extension(lib, "vct_voxelize_dynamic_device")(None, None, 12, 0, None, 0, None, None, 0) == 1
    assert _lib.bind_dynamic_extension(lib, "vct_dynamic_voxels")(None, C.byref(n)) == 1


def test_library_without_them_still_loads(oracle_mod):
    """The CPU backend exports vct.h only: it binds, runs, and refuses the new calls by name."""
    from helpers import scene_arrays
    from vct import Context, _lib, scenes
    cpu = _lib.bind(C.CDLL(oracle_mod.CPU_BACKEND))
    for name in NAMES:
        assert not hasattr(cpu, name)
        with pytest.raises(AttributeError, match=name):
            _lib.bind_dynamic_extension(cpu, name)
    s, (v, i, m, k) = scene_arrays("cornell")
    g0, E = scenes.grid_for_unit_box(16)
    ctx = Context(16, g0, E, lib=cpu)
    ctx.voxelize(v, i, m, k)
    before = ctx.download_accum()
    with pytest.raises(AttributeError, match="vct_voxelize_dynamic"):
        ctx.voxelize_dynamic(*D.layers()["floor"])
    with pytest.raises(AttributeError, match="vct_dynamic_voxels"):
        ctx.dynamic_voxels()
    after = ctx.download_accum()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    ctx.close()


def test_binding_checks_shapes_before_the_library():
    """Argument errors the binding can see are VctError(EINVAL) without a context call."""
    from vct import Context, VctError
    ctx = Context.__new__(Context)          # no vct_create: the checks come before any library call
    from vct import _lib
    ctx.lib, ctx.h = _lib.load(), None
    v, i, m, k = D.layers()["floor"]
    for args in ((v, i[:-1], m, k), (v, i, m[:-1], k), (v, i, m, k[:, :3]), (v[:, :2], i, m, k)):
        with pytest.raises(VctError) as e:
            ctx.voxelize_dynamic(*args)
        assert e.value.status == 1


# ---- the host ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["1,2", "1,2,3,4", "a,b,c", "1,,3", "nan,1,1", "1,inf,1", "", "1 2 3", "1,2,3,"])
def test_host_refuses_a_malformed_dynamic_offset(spec):
    assert os.path.exists(EXE), "build the host with `make -C voxel-based-global-illumination_amd host`"
    p = subprocess.run([EXE, "none.obj", "--dynamic", "box.obj", f"--dynamic-offset={spec}"], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 2 and "malformed --dynamic-offset" in p.stderr, (p.returncode, p.stderr)


def test_host_refuses_dynamic_without_a_file():
    assert os.path.exists(EXE)
    for flags in (["--dynamic"], ["--dynamic="], ["--dynamic-offset", "1,2,3"]):
        p = subprocess.run([EXE, "none.obj"] + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "--dynamic" in p.stderr, (flags, p.returncode, p.stderr)


def test_host_accepts_dynamic_flags_before_it_needs_the_models():
    """Well-formed flags get as far as the missing model (exit 1, not the usage error)."""
    assert os.path.exists(EXE)
    for flags in (["--dynamic", "box.obj"], ["--dynamic=box.obj", "--dynamic-offset", "0.5,-1,2e-1"],
                  ["--dynamic", "box.obj", "--dynamic-offset=0,0,0"]):
        p = subprocess.run([EXE, "none.obj"] + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "cannot open" in p.stderr, (flags, p.returncode, p.stderr)
