"""Frames for the HDR present (include/vct_present.h), every one built from a seed: an HDR ramp, a
constant frame, a frame that populates every bin of the meter, and a hostile frame.  The sizes
are the smallest at which a kernel can still go wrong: one pixel, a frame smaller than any tile,
odd sizes, one of several blocks whose bloom levels are odd at several steps."""
import numpy as np

import present_ref as PR

F = np.float32
SIZES = ((1, 1), (3, 5), (17, 9), (64, 64), (130, 70))          # (w, h)
CONSTANT = (3.0, 2.0, 0.5)


def ramp(w, h, seed=1):
    """Luminances spread log-uniformly over 2^-20 .. 2^20 with a random chroma, alpha 1."""
    rng = np.random.default_rng([seed, w, h])
    lum = np.exp2(rng.uniform(-20.0, 20.0, (h, w)))
    chroma = rng.uniform(0.25, 1.0, (h, w, 3))
    out = np.ones((h, w, 4), F)
    out[..., :3] = (lum[..., None] * chroma).astype(F)
    return out


def constant(w, h, rgb=CONSTANT):
    out = np.ones((h, w, 4), F)
    out[..., :3] = np.array(rgb, F)
    return out


def every_bin(w, h):
    """Grey pixels at the centres of the keys KEY0 - 1 .. KEY0 + 512 in turn (the first is under,
    the last over): w * h >= 514 populates every bin.  A centre keeps the rounding of Y's three
    operations well inside its bin."""
    j = np.arange(w * h) % (PR.BINS + 2)
    bits = ((PR.KEY0 - 1 + j) << 19) + (1 << 18)
    grey = bits.astype(np.uint32).view(F).reshape(h, w)
    out = np.ones((h, w, 4), F)
    out[..., :3] = grey[..., None]
    return out


HOSTILE_VALUES = (np.nan, np.inf, -np.inf, -1.5, -0.0, 1e-42, 3e-39, 0.0, 3e38, 65536.0, 2.0 ** -16)


def hostile(w, h, seed=2):
    """The ramp (narrowed to 2^-8 .. 2^8) with specials in single channels, whole pixels of
    specials, backgrounds with a = 0 and a = -0.0f (over garbage rgb) and odd alphas, scattered so
    that the first wave of every size holds several kinds."""
    rng = np.random.default_rng([seed, w, h])
    out = np.ones((h, w, 4), F)
    out[..., :3] = (np.exp2(rng.uniform(-8.0, 8.0, (h, w, 1))) * rng.uniform(0.25, 1.0, (h, w, 3))).astype(F)
    flat = out.reshape(-1, 4)
    n = flat.shape[0]
    kind = rng.integers(0, 8, n)
    kind[: min(n, 8)] = np.arange(min(n, 8))           # the first pixels: one of each
    special = np.array(HOSTILE_VALUES, F)
    for i in range(n):
        k = kind[i]
        if k == 1:
            flat[i, rng.integers(0, 3)] = special[rng.integers(0, special.size)]
        elif k == 2:
            flat[i, :3] = special[rng.integers(0, special.size, 3)]
        elif k == 3:
            flat[i, 3] = 0.0
        elif k == 4:
            flat[i, 3] = -0.0
            flat[i, :3] = special[rng.integers(0, special.size, 3)]
        elif k == 5:
            flat[i, 3] = (0.5, np.nan, -1.0, np.inf)[rng.integers(0, 4)]
    return out


def catalogue():
    """[(name, frame)] over every size: what the CPU and the GPU tests share."""
    out = []
    for w, h in SIZES:
        for name, make in (("ramp", ramp), ("constant", constant), ("every_bin", every_bin), ("hostile", hostile)):
            out.append((f"{name}_{w}x{h}", make(w, h)))
    return out


# (curve, white, transfer) of the present's configurations under test
CONFIGS = ((PR.REINHARD, 1.0, PR.GAMMA22), (PR.REINHARD_WHITE, 4.0, PR.SRGB), (PR.ACES, 1.0, PR.SRGB), (PR.CLAMP, 1.0, PR.GAMMA22))

# The largest difference between the device's and libm's transfer value t (powf) over the catalogue,
# every configuration and the Cornell frame, as tests/test_present_gpu.py measures and prints it on
# the MI355X: 1.192e-07, one unit of the last place of a t just below 1.  255 x this is the band
# around a floor threshold inside which a dithered byte may differ by 1.
DEVICE_T_DIFF = 2.0 ** -23
