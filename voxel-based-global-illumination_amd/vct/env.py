"""Environment maps for include/vct_env.h: the octahedral layout on the host, and EnvMap.

The C ABI takes one octahedral square of RGBA float texels (vct_set_env) and a per-call record
(vct_env_sky: frame and scale).  EnvMap keeps both, and the helpers here fill the square from
what a user has: an equirectangular panorama, a vct_sky, or a function of the direction.  They
evaluate the texel-centre directions in float64 and are convenience: the bit-exact contract
(include/vct_spec.h "environment sky") starts at the texels they produce.

Layout: texel (x, y) has its centre at p = ((x + 0.5) * 2 / S - 1, (y + 0.5) * 2 / S - 1); a
map-space unit direction e lies at p = (e.x, e.y) / (|e.x| + |e.y| + |e.z|), folded over the
diamond |p.x| + |p.y| = 1 when e.z < 0.  The record's frame rows are the world directions of
the map's x, y and z axes, so a world direction d has e_c = frame[c] . d.
"""
from __future__ import annotations

import numpy as np

from . import env_sky

# the default frame: the map's +z is the world's +y, so the upper hemisphere is the inner diamond
Y_UP = ((1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))


def oct_decode(p):
    """p [..., 2] in [-1, 1]^2 -> map-space unit directions [..., 3] (float64)."""
    p = np.asarray(p, np.float64)
    z = 1.0 - np.abs(p[..., 0]) - np.abs(p[..., 1])
    x = np.where(z < 0, (1.0 - np.abs(p[..., 1])) * np.copysign(1.0, p[..., 0]), p[..., 0])
    y = np.where(z < 0, (1.0 - np.abs(p[..., 0])) * np.copysign(1.0, p[..., 1]), p[..., 1])
    e = np.stack([x, y, z], axis=-1)
    return e / np.linalg.norm(e, axis=-1, keepdims=True)


def oct_encode(e):
    """Map-space directions [..., 3] -> p [..., 2] (float64), the inverse of oct_decode."""
    e = np.asarray(e, np.float64)
    p = e[..., :2] / np.abs(e).sum(axis=-1, keepdims=True)
    q = (1.0 - np.abs(p[..., ::-1])) * np.copysign(1.0, p)
    return np.where(e[..., 2:3] < 0, q, p)


def texel_dirs(size: int, frame=Y_UP):
    """World unit directions of the size x size texel centres, [size, size, 3] float64."""
    c = (np.arange(size) + 0.5) * 2.0 / size - 1.0
    e = oct_decode(np.stack(np.meshgrid(c, c, indexing="xy"), axis=-1))
    return e @ np.asarray(frame, np.float32).astype(np.float64)      # frame is orthonormal: d = frame^T e


class EnvMap:
    """An octahedral map with the record that goes with it.

    texels: [S, S, 4] float32 (S a power of two); frame, scale: the vct_env_sky fields.
    upload(ctx) hands the texels to the context; the calls take the EnvMap where they take a
    record (ctx.env_cones_device(..., env_map, ...)), or `record` directly."""

    def __init__(self, texels, frame=Y_UP, scale: float = 1.0):
        t = np.ascontiguousarray(texels, dtype=np.float32)
        if t.ndim == 3 and t.shape[2] == 3:
            t = np.concatenate([t, np.ones(t.shape[:2] + (1,), np.float32)], axis=2)
        s = t.shape[0]
        if t.ndim != 3 or t.shape[1] != s or t.shape[2] != 4 or s < 1 or s & (s - 1):
            raise ValueError(f"EnvMap: texels must be [S, S, 3 or 4] with S a power of two, got {t.shape}")
        self.texels = t
        self.frame = tuple(tuple(float(v) for v in row) for row in frame)
        self.scale = float(scale)

    @property
    def size(self) -> int:
        return self.texels.shape[0]

    @property
    def record(self):
        return env_sky(self.frame, self.scale)

    def upload(self, ctx):
        ctx.set_env(self.texels)
        return self

    # ---- host helpers ------------------------------------------------------------------------
    @classmethod
    def from_function(cls, fn, size: int, frame=Y_UP, scale: float = 1.0):
        """fn(d) -> rgb for world unit directions d [size, size, 3] (float64), evaluated at the
        texel centres."""
        rgb = np.asarray(fn(texel_dirs(size, frame)), np.float64)
        return cls(np.broadcast_to(rgb, (size, size, 3)).astype(np.float32), frame, scale)

    @classmethod
    def from_sky(cls, sky, size: int, frame=Y_UP, scale: float = 1.0):
        """The three-colour sky of include/vct_sky.h (a VctSky, or a dict of up / zenith / horizon /
        ground) sampled at the texel centres."""
        get = (lambda k: sky[k]) if isinstance(sky, dict) else (lambda k: list(getattr(sky, k)))
        up = np.asarray(get("up"), np.float64)
        up = up / np.linalg.norm(up)
        z, h, g = (np.asarray(get(k), np.float64) for k in ("zenith", "horizon", "ground"))

        def colour(d):
            u = d @ up
            s_up, s_dn = np.clip(u, 0.0, 1.0)[..., None], np.clip(-u, 0.0, 1.0)[..., None]
            return (h + (z - h) * s_up) + (g - h) * s_dn
        return cls.from_function(colour, size, frame, scale)

    @classmethod
    def from_equirect(cls, img, size: int, frame=Y_UP, scale: float = 1.0):
        """An equirectangular panorama [H, W, 3 or 4] (row 0 = straight up = world +y, column 0 =
        world -z, longitude growing toward +x), sampled bilinearly at the texel centres."""
        img = np.asarray(img, np.float64)[..., :3]
        hh, ww = img.shape[:2]
        d = texel_dirs(size, frame)
        u = (np.arctan2(d[..., 0], -d[..., 2]) / (2.0 * np.pi)) % 1.0 * ww - 0.5
        v = np.arccos(np.clip(d[..., 1], -1.0, 1.0)) / np.pi * hh - 0.5
        x0, y0 = np.floor(u), np.floor(v)
        fu, fv = (u - x0)[..., None], (v - y0)[..., None]
        x0, x1 = x0.astype(np.int64) % ww, (x0.astype(np.int64) + 1) % ww            # longitude wraps
        y0, y1 = np.clip(y0.astype(np.int64), 0, hh - 1), np.clip(y0.astype(np.int64) + 1, 0, hh - 1)
        top = img[y0, x0] * (1.0 - fu) + img[y0, x1] * fu
        bot = img[y1, x0] * (1.0 - fu) + img[y1, x1] * fu
        return cls((top * (1.0 - fv) + bot * fv).astype(np.float32), frame, scale)
