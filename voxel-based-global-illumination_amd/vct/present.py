"""The HDR present (include/vct_present.h) around a :class:`vct.Context`.

:class:`Presenter` owns what the four calls need between frames -- the histogram, the two
exposure records (swapped each frame), the bloom scratch -- and queues meter -> exposure update
-> bloom -> present on the context's stream.  Nothing is read back: the metered exposure stays on
the device.  The buffers are torch tensors on the context's device.
"""
from __future__ import annotations

import ctypes as C
import math

from . import VctError, _lib
from ._lib import VctBloomParams, VctExposureParams, VctPresentParams

_EINVAL = 1
TRANSFERS = {"gamma22": _lib.VCT_TRANSFER_GAMMA22, "srgb": _lib.VCT_TRANSFER_SRGB}


def adaptation_rate(dt: float, speed: float) -> float:
    """1 - exp(-dt * speed), the blend weight of one frame of `dt` seconds, in [0, 1]."""
    return min(max(-math.expm1(-max(float(dt), 0.0) * max(float(speed), 0.0)), 0.0), 1.0)


def bloom_sizes(width: int, height: int, levels: int):
    """[(w_k, h_k)] of the bloom levels 1 .. L of a width x height frame (vct_bloom_scratch_bytes)."""
    out, w, h = [], width, height
    for k in range(levels):
        if k > 0 and (w, h) == (1, 1):
            break
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


class Presenter:
    """curve: a key of _lib.VCT_CURVES; transfer: "gamma22" or "srgb".  exposure=None meters the
    frame (auto-exposure, adapting with speed_up / speed_down per second), a number is a manual
    exposure.  bloom_levels=0 turns bloom off."""

    def __init__(self, ctx, width: int, height: int, curve="reinhard", transfer="gamma22", dither=False, white=4.0,
                 exposure=None, key_value=0.18, min_exposure=2.0 ** -12, max_exposure=2.0 ** 12, low_permille=100,
                 high_permille=20, speed_up=3.0, speed_down=1.0, bloom_levels=0, bloom_threshold=1.0,
                 bloom_intensity=0.25):
        import torch
        if curve not in _lib.VCT_CURVES or transfer not in TRANSFERS:
            raise VctError(_EINVAL, f"Presenter: unknown curve {curve!r} or transfer {transfer!r}")
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        self.curve, self.transfer, self.dither, self.white = _lib.VCT_CURVES[curve], TRANSFERS[transfer], bool(dither), float(white)
        self.exposure = None if exposure is None else float(exposure)
        self.key_value, self.min_exposure, self.max_exposure = float(key_value), float(min_exposure), float(max_exposure)
        self.low_permille, self.high_permille = int(low_permille), int(high_permille)
        self.speed_up, self.speed_down = float(speed_up), float(speed_down)
        self.bloom_levels, self.bloom_threshold, self.bloom_intensity = int(bloom_levels), float(bloom_threshold), float(bloom_intensity)
        dev = torch.device("cuda", ctx.device if ctx.device >= 0 else torch.cuda.current_device())
        self.hist = torch.zeros(_lib.VCT_PRESENT_BINS, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(4, dtype=torch.int32, device=dev)
        self.states = torch.zeros((2, 4), dtype=torch.float32, device=dev)     # two vct_exposure_state records
        self.cur = 0                  # the record of the last update
        self.has_state = False
        self.scratch = None
        if self.bloom_levels:
            n = C.c_size_t()
            st = self._fn("vct_bloom_scratch_bytes")(self.width, self.height, self.bloom_levels, C.byref(n))
            if st != 0:
                raise VctError(st, "vct_bloom_scratch_bytes: a frame size or level count outside its rule")
            self.scratch = torch.zeros(n.value // 4, dtype=torch.float32, device=dev)

    def _fn(self, name):
        return _lib.bind_present_extension(self.ctx.lib, name)

    def _state_ptr(self, i):
        return self.states.data_ptr() + 16 * i

    def set_exposure(self, exposure):
        """A manual exposure from the next present on; None returns to the meter."""
        self.exposure = None if exposure is None else float(exposure)
        if exposure is None:
            self.has_state = False

    def meter(self, linear4):
        """vct_luminance_meter_device into the presenter's histogram; -> (hist, counts), device tensors."""
        c = self.ctx
        n = 4 * self.width * self.height
        c._check(self._fn("vct_luminance_meter_device")(c.h, c._dev(linear4, "linear4", min_numel=n), self.width, self.height,
                                                         self.hist.data_ptr(), self.counts.data_ptr()), "luminance_meter")
        return self.hist, self.counts

    def exposure_params(self, dt: float) -> VctExposureParams:
        p = VctExposureParams()
        p.key_value, p.min_exposure, p.max_exposure = self.key_value, self.min_exposure, self.max_exposure
        p.low_permille, p.high_permille = self.low_permille, self.high_permille
        p.rate_up, p.rate_down = adaptation_rate(dt, self.speed_up), adaptation_rate(dt, self.speed_down)
        return p

    def present(self, linear4, dt: float = 1.0 / 60.0, out_display4=None, out_rgba8=None):
        """One frame: [meter -> exposure update ->] [bloom ->] present, queued on the context's
        stream.  At least one of out_display4 (float32 [h, w, 4]) and out_rgba8 (int32 [h, w])."""
        c, w, h = self.ctx, self.width, self.height
        n = 4 * w * h
        lin = c._dev(linear4, "linear4", min_numel=n)
        state = None
        if self.exposure is None:
            self.meter(linear4)
            p = self.exposure_params(dt)
            prev = self._state_ptr(self.cur) if self.has_state else None
            nxt = 1 - self.cur if self.has_state else self.cur
            c._check(self._fn("vct_exposure_update_device")(c.h, self.hist.data_ptr(), self.counts.data_ptr(), C.byref(p), prev,
                                                             self._state_ptr(nxt)), "exposure_update")
            self.cur, self.has_state = nxt, True
            state = self._state_ptr(self.cur)
        scalar = 1.0 if self.exposure is None else self.exposure
        bloom = None
        if self.bloom_levels:
            b = VctBloomParams()
            b.threshold, b.levels, b.exposure = self.bloom_threshold, self.bloom_levels, scalar
            c._check(self._fn("vct_bloom_device")(c.h, lin, w, h, C.byref(b), state, self.scratch.data_ptr(),
                                                   self.scratch.numel() * 4), "bloom")
            bloom = self.scratch.data_ptr()
        q = VctPresentParams()
        q.curve, q.transfer, q.dither = self.curve, self.transfer, int(self.dither)
        q.exposure, q.white, q.bloom_intensity = scalar, self.white, self.bloom_intensity
        c._check(self._fn("vct_present_device")(c.h, lin, w, h, C.byref(q), state, bloom,
                                                 c._dev(out_display4, "out_display4", min_numel=n),
                                                 c._dev(out_rgba8, "out_rgba8", ("torch.int32", "torch.uint32"), w * h)), "present")
        return out_display4, out_rgba8
