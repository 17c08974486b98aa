"""The voxel view and ray picking of include/vct_voxview.h, returning tensors.

    frame = voxview.view(ctx, cam, 1920, 1080, level=0, mode="radiance", shade=True)
    frame["linear"], frame["rgba8"], frame["hit"], frame["cells"]

    hits = voxview.pick(ctx, origins, dirs)            # K1's occupancy, level 0
    hits["cell"], hits["face"], hits["steps"], hits["t"], hits["hit"]

Device work is queued on the context's stream; reading `cells` (a Python int) waits for it.
"""
from __future__ import annotations

import numpy as np

from . import VctError, _EINVAL, _lib

MODES = _lib.VCT_VOXVIEW_MODES
SOLID = {"occupancy": _lib.VCT_VOXPICK_OCCUPANCY, "alpha": _lib.VCT_VOXPICK_ALPHA}


def _device(ctx):
    return f"cuda:{ctx.device}" if ctx.device >= 0 else "cuda"


def _enum(value, names, what):
    if isinstance(value, str):
        if value not in names:
            raise VctError(_EINVAL, f"{what}: {value!r} is none of {', '.join(names)}")
        return names[value]
    return int(value)


def split_hits(hit4):
    """An int32 tensor [..., 4] of hit records -> dict(cell, face, steps: int64 tensors, t: float32,
    hit: bool).  A miss has cell -1 here (0xFFFFFFFF in the record)."""
    import torch
    h = hit4.to(torch.int32)
    cell = h[..., 0].to(torch.int64)
    return {"cell": cell, "face": h[..., 1].to(torch.int64), "steps": h[..., 2].to(torch.int64),
            "t": h[..., 3].contiguous().view(torch.float32), "hit": cell >= 0}


def view(ctx, cam, w, h, level=0, mode="radiance", shade=False, count_cells=True):
    """The voxel view of `cam` (a vct.camera.Camera or VctCamera) at w x h: dict(linear
    [h, w, 4] float32, rgba8 [h, w] int32, hit [h, w, 4] int32 device tensors, and cells, the
    number of cells the frame tested, when count_cells)."""
    import torch
    dev = _device(ctx)
    lin = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
    rgba = torch.empty((h, w), dtype=torch.int32, device=dev)
    hit = torch.empty((h, w, 4), dtype=torch.int32, device=dev)
    cells = torch.zeros(1, dtype=torch.int64, device=dev) if count_cells else None
    ctx.voxel_view_device(cam, w, h, level, _enum(mode, MODES, "voxview.view mode"), shade, lin, rgba, hit, cells)
    out = {"linear": lin, "rgba8": rgba, "hit": hit}
    if count_cells:
        out["cells"] = int(cells.item())
    return out


def pick(ctx, origins, dirs, t_lim=None, level=0, solid="occupancy", count_cells=False):
    """Walks rays through `level`: origins, dirs array-likes or tensors [R, 3] (world units; any
    length of direction), t_lim [R] in level-0 voxel units (default: no limit).  -> the dict of
    split_hits over the R rays, with `record` the raw int32 [R, 4] tensor (and cells)."""
    import torch
    dev = _device(ctx)
    o = torch.as_tensor(np.asarray(origins, np.float32) if not torch.is_tensor(origins) else origins,
                        dtype=torch.float32, device=dev).reshape(-1, 3)
    d = torch.as_tensor(np.asarray(dirs, np.float32) if not torch.is_tensor(dirs) else dirs,
                        dtype=torch.float32, device=dev).reshape(-1, 3)
    if o.shape != d.shape:
        raise VctError(_EINVAL, f"voxview.pick: {o.shape[0]} origins for {d.shape[0]} directions")
    R = o.shape[0]
    org4 = torch.zeros((R, 4), dtype=torch.float32, device=dev)
    dir4 = torch.full((R, 4), float("inf"), dtype=torch.float32, device=dev)
    org4[:, :3] = o
    dir4[:, :3] = d
    if t_lim is not None:
        dir4[:, 3] = torch.as_tensor(t_lim, dtype=torch.float32, device=dev).reshape(-1)
    hit = torch.empty((R, 4), dtype=torch.int32, device=dev)
    cells = torch.zeros(1, dtype=torch.int64, device=dev) if count_cells else None
    ctx.voxel_pick_device(org4, dir4, R, hit, level, _enum(solid, SOLID, "voxview.pick solid"), cells)
    out = split_hits(hit)
    out["record"] = hit
    if count_cells:
        out["cells"] = int(cells.item())
    return out
