"""The pose snapshot a host keeps for include/vct_motion.h.

vct_objects_motion_device is stateless: last frame's poses are the caller's.
:class:`MotionTracker` owns them for one object set and one frame size, together with the two
planes the call writes.  Per frame:

    set.move(ids, poses)                                         # the objects that moved
    ctx.gbuffer_shaded_device(cam, w, h, rough, pos4, nrm4, alb4, ks4, tri_id=tri_id, bary2=bary2)
    motion4, prev_nrm4 = tracker.planes(pos4, nrm4, tri_id, bary2)
    ... inject, build_mips, trace ...
    history.accumulate((pos4, nrm4), cam, [diffuse4], motion=motion4, test_normals=prev_nrm4)
    tracker.end_frame()                                          # the snapshot for the next frame

Before the first `end_frame` the snapshot is all zero: every object counts as hidden last frame,
so its pixels reset.  The planes belong to the tracker and are overwritten by the next call.
Device work is queued on the context's stream.
"""
from __future__ import annotations


class MotionTracker:
    def __init__(self, ctx, object_set, width: int, height: int, stats: bool = False):
        """object_set: the vct.objects.ObjectSet defined on `ctx` (or its object count).
        stats: keep the {valid, static_or_unmoved, moved, appeared} of the last frame in
        `self.stats` (a 4-element int32 device tensor)."""
        import torch
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.n_objects = object_set if isinstance(object_set, int) else len(object_set)
        dev = f"cuda:{ctx.device}" if ctx.device >= 0 else "cuda"
        self.snapshot = torch.zeros((max(self.n_objects, 1), 80), dtype=torch.uint8, device=dev)
        self.motion4 = torch.zeros((height, width, 4), dtype=torch.float32, device=dev)
        self.prev_nrm4 = torch.zeros((height, width, 4), dtype=torch.float32, device=dev)
        self.stats = torch.zeros(4, dtype=torch.int32, device=dev) if stats else None

    def planes(self, pos4, nrm4, tri_id, bary2):
        """-> (motion4, prev_nrm4) of this frame's shaded-pass planes against the snapshot."""
        self.ctx.objects_motion_device(self.width, self.height, pos4, tri_id, bary2, self.snapshot, self.motion4,
                                       nrm4=nrm4, prev_nrm4=self.prev_nrm4, stats=self.stats, n_prev=self.n_objects)
        return self.motion4, self.prev_nrm4

    def end_frame(self):
        """Take the snapshot: the set's poses as they stand are `last frame's` from now on."""
        self.ctx.objects_poses_device(self.snapshot)
