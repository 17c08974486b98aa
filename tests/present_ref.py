"""The HDR present of include/vct_present.h restated in numpy, operation for operation
(include/vct_spec.h "present"): the luminance meter, the exposure update (python integers), the
bloom chain, the curves in float32 and, as an anchor, in float64, the transfer functions and the
two quantisations.  tests/test_present.py checks its properties on the CPU;
tests/test_present_gpu.py compares csrc/vct_present.hip with it bit for bit."""
import numpy as np

from shading_ref import fmaf32

F = np.float32
BINS, KEY0 = 512, (127 - 16) << 4
MAX_LEVELS = 8
REINHARD, REINHARD_WHITE, ACES, CLAMP = 0, 1, 2, 3
GAMMA22, SRGB = 0, 1
INV_GAMMA, SRGB_INV_GAMMA = F(0.454545468), F(0.416666657)
CLEAR = np.array([0.2, 0.3, 0.3], F)
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.int64)


def luma(lin):
    lin = np.asarray(lin, F)
    with np.errstate(all="ignore"):
        return fmaf32(F(0.0722), lin[..., 2], fmaf32(F(0.7152), lin[..., 1], F(0.2126) * lin[..., 0]))


def background(lin):
    return np.asarray(lin, F)[..., 3] == 0          # also -0.0f


def key_of(y):
    """bits(Y) >> 19 of float32 values that the meter counts."""
    return np.asarray(y, F).view(np.uint32).astype(np.int64) >> 19


def meter(lin):
    """-> (hist [512] uint32, counts [4] uint32 = counted, under, over, rejected)."""
    y = luma(lin).reshape(-1)[~background(lin).reshape(-1)]
    bits = y.view(np.uint32).astype(np.int64)
    rejected = bits >= 0x7F800000                     # Inf, NaN, or the sign bit
    d = (bits[~rejected] >> 19) - KEY0
    hist = np.bincount(np.clip(d, 0, BINS - 1), minlength=BINS).astype(np.uint32)
    return hist, np.array([d.size, (d < 0).sum(), (d > BINS - 1).sum(), rejected.sum()], np.uint32)


def bin_centre(m256):
    """float_from_bits((KEY0 << 19) + (M << 11) + (1 << 18)), M the bin in 1/256."""
    return np.array([(KEY0 << 19) + (int(m256) << 11) + (1 << 18)], np.uint32).view(F)[0]


class ExposureParams:
    def __init__(self, key_value=0.18, min_exposure=2.0 ** -12, max_exposure=2.0 ** 12, low_permille=0, high_permille=0,
                 rate_up=1.0, rate_down=1.0):
        self.key_value, self.min_exposure, self.max_exposure = F(key_value), F(min_exposure), F(max_exposure)
        self.low_permille, self.high_permille = int(low_permille), int(high_permille)
        self.rate_up, self.rate_down = F(rate_up), F(rate_down)


def trimmed(hist, counted, low_permille, high_permille):
    """(n, S) of the bins kept after the two trims, python integers."""
    keep = [int(v) for v in hist]
    lo, hi = int(counted) * low_permille // 1000, int(counted) * high_permille // 1000
    for b in range(BINS):
        t = min(keep[b], lo)
        keep[b] -= t
        lo -= t
    for b in range(BINS - 1, -1, -1):
        t = min(keep[b], hi)
        keep[b] -= t
        hi -= t
    return sum(keep), sum(b * k for b, k in enumerate(keep))


def exposure_update(hist, counts, p, prev=None):
    """-> the record (exposure, target, mean_luminance: float32; counted: int).  prev: the previous
    record's exposure (any float, also a poisoned one) or None."""
    counted = int(counts[0])
    n, S = trimmed(hist, counted, p.low_permille, p.high_permille)
    has_prev = prev is not None and np.isfinite(F(prev)) and F(prev) > 0
    prev = F(prev) if has_prev else F(1.0)
    if n == 0:
        return prev, prev, F(0.0), counted
    mean = bin_centre((S * 256) // n)
    with np.errstate(all="ignore"):
        target = p.key_value / mean
        target = p.min_exposure if target < p.min_exposure else (p.max_exposure if target > p.max_exposure else target)
        if not has_prev:
            return target, target, mean, counted
        rate = p.rate_up if target > prev else p.rate_down
        exposure = target if rate == F(1.0) else prev + (target - prev) * rate
    return F(exposure), F(target), mean, counted


def state_words(state):
    """The 16-byte record as four uint32 words."""
    e, t, m, c = state
    return np.concatenate([np.array([e, t, m], F).view(np.uint32), np.array([c & 0xFFFFFFFF], np.uint32)])


# ---- bloom ------------------------------------------------------------------------------------
def bloom_sizes(w, h, levels):
    """[(w_k, h_k)] of the levels 1 .. L."""
    out = []
    for k in range(levels):
        if k > 0 and (w, h) == (1, 1):
            break
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def natural_levels(w, h):
    return len(bloom_sizes(w, h, MAX_LEVELS))


def contribution(lin, E, threshold):
    lin = np.asarray(lin, F)
    with np.errstate(all="ignore"):
        ye = luma(lin) * F(E)
        pos = ye > 0
        wgt = np.where(pos, np.maximum(ye - F(threshold), F(0)) / np.where(pos, ye, F(1)), F(0)).astype(F)
        c = lin[..., :3] * wgt[..., None]
    ok = np.isfinite(wgt) & np.isfinite(c).all(-1) & ~background(lin)
    out = np.zeros(lin.shape, F)
    out[..., :3] = np.where(ok[..., None], c, F(0))
    return out


def box(P):
    h, w = P.shape[:2]
    oy, ox = np.arange((h + 1) // 2), np.arange((w + 1) // 2)
    y0, y1, x0, x1 = np.minimum(2 * oy, h - 1), np.minimum(2 * oy + 1, h - 1), np.minimum(2 * ox, w - 1), np.minimum(2 * ox + 1, w - 1)
    with np.errstate(all="ignore"):
        out = ((P[y0][:, x0] + P[y0][:, x1]) + (P[y1][:, x0] + P[y1][:, x1])) * F(0.25)
    out[..., 3] = 0
    return out


def up2(P, fw, fh):
    """The 2x bilinear of P at the texels of the finer level (fw x fh): weights 9, 3, 3, 1 over 16."""
    ph, pw = P.shape[:2]
    x, y = np.arange(fw), np.arange(fh)
    nx, ny = np.minimum(x >> 1, pw - 1), np.minimum(y >> 1, ph - 1)
    fx = np.clip(nx + np.where(x & 1, 1, -1), 0, pw - 1)
    fy = np.clip(ny + np.where(y & 1, 1, -1), 0, ph - 1)
    with np.errstate(all="ignore"):
        lerp = lambda a, b: fmaf32(b - a, F(0.25), a)
        out = lerp(lerp(P[ny][:, nx], P[ny][:, fx]), lerp(P[fy][:, nx], P[fy][:, fx])).astype(F)
    out[..., 3] = 0
    return out


def bloom(lin, E, threshold, levels):
    """-> (D, U): the down and the up chain, lists over the levels 1 .. L."""
    h, w = lin.shape[:2]
    sizes = bloom_sizes(w, h, levels)
    D = [box(contribution(lin, E, threshold))]
    for _ in sizes[1:]:
        D.append(box(D[-1]))
    assert [(d.shape[1], d.shape[0]) for d in D] == sizes
    U = [None] * len(D)
    U[-1] = D[-1]
    for k in range(len(D) - 2, -1, -1):
        with np.errstate(all="ignore"):
            U[k] = D[k] + up2(U[k + 1], D[k].shape[1], D[k].shape[0])
        U[k][..., 3] = 0
    return D, U


# ---- present ----------------------------------------------------------------------------------
def curve(v, which, white=1.0, dtype=F):
    """The curve on sanitised values v >= 0 (+Inf allowed), in `dtype` arithmetic."""
    T = dtype
    v = np.asarray(v, T)
    one = T(1)
    fma = fmaf32 if dtype is F else (lambda a, b, c: np.asarray(a, T) * b + c)
    with np.errstate(all="ignore"):
        if which == REINHARD:
            d = v / (one + v)
        elif which == REINHARD_WHITE:
            w2 = T(F(white) * F(white)) if dtype is F else T(F(white)) * T(F(white))
            d = (v * (one + v / w2)) / (one + v)
            d = np.where(d < one, d, one)
        elif which == ACES:
            d = (v * fma(T(F(2.51)), v, T(F(0.03)))) / fma(v, fma(T(F(2.43)), v, T(F(0.59))), T(F(0.14)))
            d = np.where(d < one, d, one)
        else:
            d = np.where(v < one, v, one)
    return np.where(np.isposinf(v), one, d).astype(T)


def display(lin, E, which, white=1.0, bloom_u1=None, intensity=0.0, dtype=F):
    """out_display4.  dtype=np.float64: the same formulas on the same float32 inputs in float64
    (every product and sum unrounded to float32)."""
    lin = np.asarray(lin, F)
    h, w = lin.shape[:2]
    T = dtype
    with np.errstate(all="ignore"):
        v = lin[..., :3].astype(T) * T(F(E))
        if bloom_u1 is not None:
            b = up2(bloom_u1, w, h)[..., :3] if dtype is F else up2_64(bloom_u1, w, h)[..., :3]
            v = fmaf32(b, F(intensity), v) if dtype is F else b * T(F(intensity)) + v
        v = np.where(v > 0, v, T(0))
    out = np.empty(lin.shape, T)
    out[..., :3] = curve(v, which, white, dtype)
    bg = background(lin)
    out[bg, :3] = CLEAR.astype(T)
    out[..., 3] = lin[..., 3]
    if dtype is F:                                     # alpha is copied: keep its bits (-0.0f, a NaN's payload)
        out.view(np.uint32)[..., 3] = lin.view(np.uint32)[..., 3]
    return out


def up2_64(P, fw, fh):
    P = np.asarray(P, np.float64)
    ph, pw = P.shape[:2]
    x, y = np.arange(fw), np.arange(fh)
    nx, ny = np.minimum(x >> 1, pw - 1), np.minimum(y >> 1, ph - 1)
    fx = np.clip(nx + np.where(x & 1, 1, -1), 0, pw - 1)
    fy = np.clip(ny + np.where(y & 1, 1, -1), 0, ph - 1)
    lerp = lambda a, b: (b - a) * 0.25 + a
    with np.errstate(all="ignore"):
        return lerp(lerp(P[ny][:, nx], P[ny][:, fx]), lerp(P[fy][:, nx], P[fy][:, fx]))


def transfer(d, which):
    """The transfer function on curve outputs, float32 (powf is libm's here, the device's there)."""
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        if which == GAMMA22:
            return np.power(d, INV_GAMMA).astype(F)
        return np.where(d <= F(0.0031308), d * F(12.92), fmaf32(F(1.055), np.power(d, SRGB_INV_GAMMA), F(-0.055))).astype(F)


def dither_offsets(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return ((BAYER[y & 3, x & 3].astype(F) + F(0.5)) / F(16.0)).astype(F)


def quant8(t):
    """clamp(lroundf(t * 255.0f), 0, 255): half away from zero."""
    with np.errstate(all="ignore"):
        x = (np.asarray(t, F) * F(255.0)).astype(np.float64)
    return np.clip(np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5)), 0, 255).astype(np.uint32)


def dither_f(t, w, h):
    """f = fmaf(t, 255, (B + 0.5) / 16) per channel of t [h, w, 3]."""
    return fmaf32(np.asarray(t, F), F(255.0), dither_offsets(w, h)[..., None])


def pack(q, bg):
    """[h, w, 3] bytes -> RGBA8 words, the clear colour at the background pixels."""
    q = np.asarray(q, np.uint32).copy()
    q[bg] = quant8(CLEAR)
    return q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | np.uint32(255 << 24)


def rgba8(disp, lin, which, dither=False):
    """out_rgba8 from a display frame (the reference's own, or the device's)."""
    h, w = disp.shape[:2]
    t = transfer(disp[..., :3], which)
    q = np.clip(np.floor(dither_f(t, w, h).astype(np.float64)), 0, 255).astype(np.uint32) if dither else quant8(t)
    return pack(q, background(lin))


def unpack(words):
    w = np.asarray(words).view(np.uint32)
    return np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24], -1).astype(np.int64)
