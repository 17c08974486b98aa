"""The probe grid a host keeps for include/vct_query.h.

vct_probe_build_device and vct_probe_sample_device are stateless: the probes and their states
are the caller's.  :class:`ProbeGrid` owns the two tensors of one grid.

    grid = ProbeGrid.over_aabb(ctx, 32)          # 32^3 probes over the context's AABB
    after every relight (inject -> build_mips [-> bounces]):
        grid.build()
    for every frame, for the points the G-buffer's trace does not light:
        plane = grid.sample(pos4, nrm4)          # the meaning of K4's diffuse4
        ... composite with plane ...

Device work is queued on the context's stream.
"""
from __future__ import annotations

import numpy as np

from . import VctError, _EINVAL, probe_grid


class ProbeGrid:
    def __init__(self, ctx, origin, spacing: float, dims):
        """Probe (i, j, k) stands at origin + (i, j, k) * spacing; dims = (dx, dy, dz), each in
        1 .. 256."""
        import torch
        self.ctx = ctx
        self.grid = probe_grid(origin, spacing, dims)
        dx, dy, dz = (int(v) for v in self.grid.dims)
        if not (all(1 <= v <= 256 for v in (dx, dy, dz)) and np.isfinite(self.grid.spacing) and self.grid.spacing > 0
                and all(np.isfinite(v) for v in self.grid.origin)):
            raise VctError(_EINVAL, f"ProbeGrid: origin {tuple(origin)}, spacing {spacing}, dims {tuple(dims)} "
                                    "break the input rule (finite origin, spacing > 0, dims in 1 .. 256)")
        dev = f"cuda:{ctx.device}" if ctx.device >= 0 else "cuda"
        self.probes = torch.zeros((dz, dy, dx, 6, 4), dtype=torch.float32, device=dev)
        self.state = torch.zeros((dz, dy, dx), dtype=torch.int32, device=dev)
        self.misses = torch.zeros(1, dtype=torch.int32, device=dev)
        self.built = False

    @classmethod
    def over_aabb(cls, ctx, d: int):
        """d probes per axis over the context's AABB, the first and last half a spacing inside
        the box (float32 arithmetic, so a C host that does the same gets the same grid)."""
        F = np.float32
        spacing = F(ctx.extent) / F(d)
        origin = np.array(ctx.aabb_min, F) + F(0.5) * spacing
        return cls(ctx, [float(v) for v in origin], float(spacing), (d, d, d))

    def build(self, cone_steps=None):
        """Trace the six cones of every probe through the context's current pyramid."""
        self.ctx.probe_build_device(self.grid, self.probes, self.state, cone_steps)
        self.built = True
        return self

    def sample(self, pos4, nrm4, out4=None):
        """pos4, nrm4: float32 device tensors [..., 4] -> out4 of pos4's shape (allocated when
        None).  `self.misses` counts the points without a valid probe around them, over every
        call since it was last zeroed."""
        import torch
        if not self.built:
            raise VctError(_EINVAL, "ProbeGrid.sample before build()")
        if out4 is None:
            out4 = torch.empty_like(pos4)
        self.ctx.probe_sample_device(self.grid, self.probes, self.state, pos4, nrm4, pos4.numel() // 4, out4, self.misses)
        return out4
