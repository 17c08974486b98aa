"""The history a host keeps for include/vct_temporal.h.

vct_temporal_accumulate_device is stateless: last frame's accumulated planes, history lengths,
G-buffer and camera are the caller's.  :class:`History` owns them for one frame size: two sets
of planes and lengths that swap every frame, a copy of the previous position and normal planes,
and the previous camera.

    hist = History(ctx, width, height, n_planes=1)
    for every frame:
        ... G-buffer, trace ...
        (diffuse_acc,) = hist.accumulate((pos4, nrm4), camera, [diffuse4])
        ... composite with diffuse_acc ...

The planes `accumulate` returns belong to the history and stay valid until the call after the
next one.  Device work is queued on the context's stream.
"""
from __future__ import annotations

import contextlib

from . import VctError, _EINVAL


class History:
    def __init__(self, ctx, width: int, height: int, n_planes: int = 1, params=None, stats: bool = False):
        """params: a VctTemporalParams (Context.temporal_params), default the header's.
        stats: keep the {valid, reused, reset_offscreen, reset_rejected} of the last frame in
        `self.stats` (a 4-element int32 device tensor)."""
        import torch
        if not 1 <= n_planes <= 4:
            raise VctError(_EINVAL, f"History: n_planes {n_planes}, expected 1 .. 4")
        self.ctx, self.width, self.height, self.n_planes = ctx, int(width), int(height), int(n_planes)
        self.params = params if params is not None else ctx.temporal_params()
        dev = f"cuda:{ctx.device}" if ctx.device >= 0 else "cuda"
        plane = lambda: torch.zeros((height, width, 4), dtype=torch.float32, device=dev)
        self._planes = [[plane() for _ in range(n_planes)] for _ in range(2)]
        self._len = [torch.zeros((height, width), dtype=torch.int32, device=dev) for _ in range(2)]
        self._gbuf = [plane(), plane()]          # last frame's position and normal planes
        self.stats = torch.zeros(4, dtype=torch.int32, device=dev) if stats else None
        self._cur = 0                            # the set the last frame wrote
        self._cam = None                         # last frame's camera; None: no history

    def reset(self):
        """Forget the history: the next frame resets every pixel (a cut, a teleport, a new scene)."""
        self._cam = None

    @property
    def planes(self):
        """The accumulated planes of the last frame."""
        return self._planes[self._cur]

    @property
    def lengths(self):
        """The history lengths of the last frame ([height, width] int32: 0 background, 1 reset)."""
        return self._len[self._cur]

    def _stream(self):
        import torch
        s = self.ctx.stream
        if s == torch.cuda.current_stream().cuda_stream:
            return contextlib.nullcontext()
        return torch.cuda.stream(torch.cuda.ExternalStream(s))

    def accumulate(self, gbuffer, camera, planes, motion=None, test_normals=None):
        """One frame.  gbuffer: (pos4, nrm4[, ...]) float32 device tensors [height, width, 4];
        camera: this frame's camera (a vct.camera.Camera or a VctCamera); planes: this frame's
        n_planes planes; motion: None, or motion4 (where each pixel's surface point was last
        frame, w = 0: nowhere); test_normals: None, or the plane the accumulate's tap tests read
        in place of nrm4 (vct.motion.MotionTracker's prev_nrm4: each pixel's normal under last
        frame's pose) -- the history still stores the real nrm4.  -> the accumulated planes."""
        planes = list(planes)
        if len(planes) != self.n_planes:
            raise VctError(_EINVAL, f"History.accumulate: {len(planes)} planes, the history holds {self.n_planes}")
        pos4, nrm4 = gbuffer[0], gbuffer[1]
        cam = camera.to_ctypes() if hasattr(camera, "to_ctypes") else camera
        old, new = self._cur, 1 - self._cur
        has = self._cam is not None
        self.ctx.temporal_accumulate_device(
            self.params, pos4, nrm4 if test_normals is None else test_normals, self.width, self.height, planes, self._planes[new], self._len[new],
            prev_cam=self._cam, prev_pos4=self._gbuf[0] if has else None, prev_nrm4=self._gbuf[1] if has else None,
            hist=self._planes[old] if has else None, hist_len=self._len[old] if has else None, motion4=motion,
            stats=self.stats)
        with self._stream():                     # after the call that read them, on the same stream
            self._gbuf[0].copy_(pos4.reshape(self.height, self.width, 4))
            self._gbuf[1].copy_(nrm4.reshape(self.height, self.width, 4))
        self._cam, self._cur = cam, new
        return self._planes[new]
