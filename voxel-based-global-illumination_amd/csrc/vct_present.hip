// vct_present.hip — the HDR present (include/vct_present.h; vct_spec.h "present"):
//  * k_meter: one float4 read per pixel, the luminance key into a 512-bin histogram kept in LDS,
//    flushed with integer global atomics (non-zero bins only).  Equal keys meet on one LDS
//    address, which the hardware takes well: a form that first folds the lanes sharing the wave's
//    first live key into one add is kept for the bench (vct_debug_present) and is not the default;
//  * k_exposure: the trimmed mean of the histogram in 64-bit integers, one wave with two
//    prefix sums, and the blend from the previous record;
//  * k_bloom_pre / k_bloom_down / k_bloom_up: plain gathers, one lane per texel of the level
//    written (only the prefilter reads a full frame);
//  * k_present: exposure, bloom (sampled from the half-resolution plane), curve, transfer,
//    quantisation.
// No float atomics anywhere, and nothing is read back.
#include <atomic>
#include "vct_internal.h"
#include "vct_view.h"

namespace vct {
namespace {

constexpr uint32_t kBins = VCT_PRESENT_BINS;
constexpr uint32_t kNone = 0xFFFFFFFFu;
// The flush is what the meter costs: every block adds its non-zero bins to the same 512 words, and a
// frame that spreads over many bins makes every block touch all of them.  So few, large blocks: 16
// waves share one LDS histogram, and at most one block per compute unit flushes.
constexpr uint32_t kMeterThreads = 1024, kMeterBlocks = 256;

__device__ __forceinline__ float luma(const float4 p) { return fmaf(0.0722f, p.z, fmaf(0.7152f, p.y, 0.2126f * p.x)); }

// ---- meter ------------------------------------------------------------------------------------
template <bool AGG>
__global__ void __launch_bounds__(kMeterThreads) k_meter(const float4* __restrict__ lin, uint32_t npx, uint32_t* hist,
                                                         uint32_t* counts) {
    __shared__ uint32_t sh[kBins + 3];      // the bins, then under, over, rejected
    for (uint32_t s = threadIdx.x; s < kBins + 3; s += kMeterThreads) sh[s] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * kMeterThreads;
    for (uint32_t base = blockIdx.x * kMeterThreads; base < npx; base += stride) {   // block-uniform trip count
        const uint32_t i = base + threadIdx.x;
        uint32_t bin = kNone, extra = kNone;
        if (i < npx) {
            const float4 p = lin[i];
            if (p.w != 0.0f) {
                const uint32_t bits = __float_as_uint(luma(p));
                if (bits >= 0x7F800000u) extra = 2u;                        // Inf, NaN, or the sign bit
                else {
                    const uint32_t key = bits >> 19;
                    if (key < VCT_PRESENT_KEY0) { bin = 0u; extra = 0u; }
                    else if (key - VCT_PRESENT_KEY0 > kBins - 1u) { bin = kBins - 1u; extra = 1u; }
                    else bin = key - VCT_PRESENT_KEY0;
                }
            }
        }
        const bool live = bin != kNone;
        if constexpr (AGG) {
            const unsigned long long lives = __ballot(live);
            if (lives) {                                                    // wave-uniform
                const int leader = __ffsll((long long)lives) - 1;
                const uint32_t lead_bin = (uint32_t)__shfl((int)bin, leader);
                const unsigned long long same = __ballot(live && bin == lead_bin);
                if ((int)lane == leader) atomicAdd(&sh[lead_bin], (uint32_t)__popcll(same));
                else if (live && bin != lead_bin) atomicAdd(&sh[bin], 1u);
            }
        } else {
            if (live) atomicAdd(&sh[bin], 1u);
        }
        for (uint32_t e = 0; e < 3u; ++e) {
            const unsigned long long m = __ballot(extra == e);
            if (m && lane == 0u) atomicAdd(&sh[kBins + e], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    uint32_t mine = 0u;
    if (threadIdx.x < kBins) {
        mine = sh[threadIdx.x];
        if (mine) atomicAdd(&hist[threadIdx.x], mine);
    }
    if (threadIdx.x < 3u) {
        const uint32_t v = sh[kBins + threadIdx.x];
        if (v) atomicAdd(&counts[1u + threadIdx.x], v);
    }
    for (int o = 32; o > 0; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o);
    if (lane == 0u && mine) atomicAdd(&counts[0], mine);
}

// ---- exposure update --------------------------------------------------------------------------
struct ExposureK {
    const uint32_t *hist, *counts;
    const vct_exposure_state* prev;
    vct_exposure_state* out;
    vct_exposure_params p;
};

__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += shfl_xor64(v, o);
    return v;
}
// the sum over the lanes below this one
__device__ __forceinline__ unsigned long long wave_below64(unsigned long long v, uint32_t lane) {
    unsigned long long inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = shfl_up64(inc, o);
        if ((int)lane >= o) inc += up;
    }
    return inc - v;
}

// One wave, eight consecutive bins a lane.  The two trims of the spec walk the bins in order; a
// lane knows from the sums of the lanes before it (after it, for the high trim) how much of a trim
// is left when the walk reaches its bins, so the result is the serial walk's in every bit.
__global__ void __launch_bounds__(64) k_exposure(const ExposureK k) {
    const uint32_t lane = threadIdx.x;
    unsigned long long keep[8], mine = 0;
    for (int j = 0; j < 8; ++j) { keep[j] = k.hist[8u * lane + j]; mine += keep[j]; }
    const unsigned long long counted = k.counts[0];
    const unsigned long long lo = counted * k.p.low_permille / 1000ull, hi = counted * k.p.high_permille / 1000ull;
    const unsigned long long below = wave_below64(mine, lane);
    unsigned long long left = lo > below ? lo - below : 0;
    mine = 0;
    for (int j = 0; j < 8; ++j) {
        const unsigned long long t = keep[j] < left ? keep[j] : left;
        keep[j] -= t; left -= t;
        mine += keep[j];
    }
    const unsigned long long above = wave_sum64(mine) - wave_below64(mine, lane) - mine;
    left = hi > above ? hi - above : 0;
    unsigned long long n = 0, S = 0;
    for (int j = 7; j >= 0; --j) {
        const unsigned long long t = keep[j] < left ? keep[j] : left;
        keep[j] -= t; left -= t;
        n += keep[j];
        S += (unsigned long long)(8u * lane + j) * keep[j];
    }
    n = wave_sum64(n);
    S = wave_sum64(S);
    if (lane != 0u) return;
    bool has_prev = false;
    float prev = 1.0f;
    if (k.prev) {
        const float e = k.prev->exposure;
        if (__builtin_isfinite(e) && e > 0.0f) { has_prev = true; prev = e; }
    }
    vct_exposure_state o;
    o.counted = (uint32_t)counted;
    if (n == 0) {
        o.exposure = o.target = prev;
        o.mean_luminance = 0.0f;
    } else {
        const unsigned long long M = (S * 256ull) / n;
        const float mean = __uint_as_float((VCT_PRESENT_KEY0 << 19) + ((uint32_t)M << 11) + (1u << 18));
        float target = k.p.key_value / mean;
        target = target < k.p.min_exposure ? k.p.min_exposure : (target > k.p.max_exposure ? k.p.max_exposure : target);
        o.target = target;
        o.mean_luminance = mean;
        if (!has_prev) o.exposure = target;
        else {
            const float rate = target > prev ? k.p.rate_up : k.p.rate_down;
            o.exposure = rate == 1.0f ? target : prev + (target - prev) * rate;
        }
    }
    *k.out = o;
}

// ---- bloom ------------------------------------------------------------------------------------
__device__ __forceinline__ float4 contribution(const float4 p, float E, float thr) {
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p.w == 0.0f) return zero;
    const float Ye = luma(p) * E;
    const float wgt = Ye > 0.0f ? fmaxf(Ye - thr, 0.0f) / Ye : 0.0f;
    const float r = p.x * wgt, g = p.y * wgt, b = p.z * wgt;
    if (!(__builtin_isfinite(wgt) && __builtin_isfinite(r) && __builtin_isfinite(g) && __builtin_isfinite(b))) return zero;
    return make_float4(r, g, b, 0.0f);
}

__device__ __forceinline__ float4 box4(const float4 a, const float4 b, const float4 c, const float4 d) {
    return make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f,
                       ((a.z + b.z) + (c.z + d.z)) * 0.25f, 0.0f);
}

struct BloomPreK {
    const float4* lin;
    const vct_exposure_state* state;
    float4* out;
    int w, h, ow, oh;
    float E, thr;
};

__global__ void __launch_bounds__(256) k_bloom_pre(const BloomPreK k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)k.ow * (uint32_t)k.oh) return;
    const int X = (int)(i % (uint32_t)k.ow), Y = (int)(i / (uint32_t)k.ow);
    const float E = k.state ? k.state->exposure : k.E;
    const int x0 = min(2 * X, k.w - 1), x1 = min(2 * X + 1, k.w - 1);
    const size_t r0 = (size_t)min(2 * Y, k.h - 1) * k.w, r1 = (size_t)min(2 * Y + 1, k.h - 1) * k.w;
    const float4 p00 = k.lin[r0 + x0], p10 = k.lin[r0 + x1], p01 = k.lin[r1 + x0], p11 = k.lin[r1 + x1];
    k.out[i] = box4(contribution(p00, E, k.thr), contribution(p10, E, k.thr), contribution(p01, E, k.thr),
                    contribution(p11, E, k.thr));
}

__global__ void __launch_bounds__(256) k_bloom_down(const float4* __restrict__ src, int sw, int shh, float4* __restrict__ dst,
                                                    int dw, int dh) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)dw * (uint32_t)dh) return;
    const int X = (int)(i % (uint32_t)dw), Y = (int)(i / (uint32_t)dw);
    const int x0 = min(2 * X, sw - 1), x1 = min(2 * X + 1, sw - 1);
    const size_t r0 = (size_t)min(2 * Y, shh - 1) * sw, r1 = (size_t)min(2 * Y + 1, shh - 1) * sw;
    dst[i] = box4(src[r0 + x0], src[r0 + x1], src[r1 + x0], src[r1 + x1]);
}

__device__ __forceinline__ float lerp25(float a, float b) { return fmaf(b - a, 0.25f, a); }

// the 2x bilinear of plane P (pw x ph) at the finer level's texel (x, y): weights 9, 3, 3, 1 over 16
__device__ __forceinline__ float4 up2(const float4* __restrict__ P, int pw, int ph, int x, int y) {
    const int nx = min(x >> 1, pw - 1), ny = min(y >> 1, ph - 1);
    const int fx = min(max(nx + ((x & 1) ? 1 : -1), 0), pw - 1), fy = min(max(ny + ((y & 1) ? 1 : -1), 0), ph - 1);
    const float4 a = P[(size_t)ny * pw + nx], b = P[(size_t)ny * pw + fx], c = P[(size_t)fy * pw + nx],
                 d = P[(size_t)fy * pw + fx];
    return make_float4(lerp25(lerp25(a.x, b.x), lerp25(c.x, d.x)), lerp25(lerp25(a.y, b.y), lerp25(c.y, d.y)),
                       lerp25(lerp25(a.z, b.z), lerp25(c.z, d.z)), 0.0f);
}

// U_k = D_k + up2(U_{k+1}), in place over D_k
__global__ void __launch_bounds__(256) k_bloom_up(float4* __restrict__ lvl, int w, int h, const float4* __restrict__ coarse,
                                                  int cw, int ch) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)w * (uint32_t)h) return;
    const float4 u = up2(coarse, cw, ch, (int)(i % (uint32_t)w), (int)(i / (uint32_t)w));
    const float4 d = lvl[i];
    lvl[i] = make_float4(d.x + u.x, d.y + u.y, d.z + u.z, 0.0f);
}

// ---- present ----------------------------------------------------------------------------------
struct PresentK {
    const float4* lin;
    const float4* bloom;                 // NULL: none
    const vct_exposure_state* state;     // NULL: E
    float4* disp;
    uint32_t* rgba8;
    uint32_t npx;
    int w, bw, bh;
    float E, white2, intensity;
    uint32_t curve, transfer, dither;
};

__device__ __forceinline__ float curve01(float v, uint32_t curve, float white2) {
    v = v > 0.0f ? v : 0.0f;
    if (v == __builtin_inff()) return 1.0f;
    float d;
    switch (curve) {
    case VCT_CURVE_REINHARD: return v / (1.0f + v);
    case VCT_CURVE_REINHARD_WHITE: d = (v * (1.0f + v / white2)) / (1.0f + v); break;
    case VCT_CURVE_ACES: d = (v * fmaf(2.51f, v, 0.03f)) / fmaf(v, fmaf(2.43f, v, 0.59f), 0.14f); break;
    default: d = v; break;
    }
    return d < 1.0f ? d : 1.0f;
}

__device__ __forceinline__ float transfer01(float d, uint32_t transfer) {
    return transfer == VCT_TRANSFER_GAMMA22
               ? powf(d, VCT_INV_GAMMA)
               : (d <= 0.0031308f ? d * 12.92f : fmaf(1.055f, powf(d, VCT_SRGB_INV_GAMMA), -0.055f));
}

// vct_debug_present_transfer: the transfer function alone, for measuring the device's powf
__global__ void __launch_bounds__(256) k_transfer(const float* __restrict__ d, uint32_t n, uint32_t transfer, float* t) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) t[i] = transfer01(d[i], transfer);
}

__device__ __forceinline__ uint32_t pack8(float d, const PresentK& k, float dith) {
    const float t = transfer01(d, k.transfer);
    if (!k.dither) return quant8(t);
    const int q = (int)floorf(fmaf(t, 255.0f, dith));
    return (uint32_t)(q < 0 ? 0 : (q > 255 ? 255 : q));
}

__constant__ const uint8_t kBayer[16] = {0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5};

// XY: the pixel's coordinates are needed (bloom or dither)
template <bool XY>
__global__ void __launch_bounds__(256) k_present(const PresentK k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k.npx) return;
    const float4 p = k.lin[i];
    if (p.w == 0.0f) {   // background: the composites' clear colour as it is
        if (k.disp) k.disp[i] = make_float4(VCT_CLEAR_R, VCT_CLEAR_G, VCT_CLEAR_B, p.w);
        if (k.rgba8)
            k.rgba8[i] = (uint32_t)lroundf(VCT_CLEAR_R * 255.0f) | ((uint32_t)lroundf(VCT_CLEAR_G * 255.0f) << 8) |
                         ((uint32_t)lroundf(VCT_CLEAR_B * 255.0f) << 16) | (255u << 24);
        return;
    }
    const float E = k.state ? k.state->exposure : k.E;
    float vr = p.x * E, vg = p.y * E, vb = p.z * E, dith = 0.0f;
    if constexpr (XY) {
        const int x = (int)(i % (uint32_t)k.w), y = (int)(i / (uint32_t)k.w);
        if (k.bloom) {
            const float4 b = up2(k.bloom, k.bw, k.bh, x, y);
            vr = fmaf(b.x, k.intensity, vr); vg = fmaf(b.y, k.intensity, vg); vb = fmaf(b.z, k.intensity, vb);
        }
        dith = ((float)kBayer[(y & 3) * 4 + (x & 3)] + 0.5f) / 16.0f;
    }
    const float dr = curve01(vr, k.curve, k.white2), dg = curve01(vg, k.curve, k.white2), db = curve01(vb, k.curve, k.white2);
    if (k.disp) k.disp[i] = make_float4(dr, dg, db, p.w);
    if (k.rgba8) k.rgba8[i] = pack8(dr, k, dith) | (pack8(dg, k, dith) << 8) | (pack8(db, k, dith) << 16) | (255u << 24);
}

// ---- host side --------------------------------------------------------------------------------
std::atomic<int> g_meter_agg{0};   // vct_debug_present: 1 folds the wave's first live key into one LDS atomic (tools/present_bench.py)

bool dims_ok(uint32_t w, uint32_t h) { return w >= 1 && h >= 1 && w <= VCT_PRESENT_MAX_DIM && h <= VCT_PRESENT_MAX_DIM; }

// finite, > 0 and <= 2^64 (a NaN fails the compares)
bool exposure_ok(float e) { return e > 0.0f && e <= VCT_EXPOSURE_LIMIT; }

struct BloomLevels {
    uint32_t n = 0;
    uint32_t w[VCT_BLOOM_MAX_LEVELS], h[VCT_BLOOM_MAX_LEVELS];
    size_t off[VCT_BLOOM_MAX_LEVELS];      // float4 offset in the scratch
    size_t texels = 0;
};

BloomLevels bloom_levels(uint32_t w, uint32_t h, uint32_t levels) {
    BloomLevels L;
    for (uint32_t k = 0; k < levels; ++k) {
        if (k > 0 && w == 1 && h == 1) break;       // the level before was 1 x 1: the chain has ended
        w = (w + 1) / 2; h = (h + 1) / 2;
        L.w[k] = w; L.h[k] = h; L.off[k] = L.texels;
        L.texels += (size_t)w * h;
        L.n = k + 1;
    }
    return L;
}

inline uint32_t blocks(size_t n) { return (uint32_t)((n + 255) / 256); }

}  // namespace
}  // namespace vct

using namespace vct;

// tool hook, not part of the headers: agg >= 0 selects the meter's form process-wide (0, the
// default: one LDS atomic per lane; 1: the first live lane's key is added once per wave);
// -> the form in force
extern "C" int vct_debug_present(int agg) {
    if (agg >= 0) g_meter_agg.store(agg ? 1 : 0);
    return g_meter_agg.load();
}

// test hook, not part of the headers: t[i] = the transfer function of d[i] (n floats on the
// device), as k_present computes it; queued on the ctx stream.  0, or -1 for a bad argument.
extern "C" int vct_debug_present_transfer(vct_ctx* c, const float* d, uint32_t n, uint32_t transfer, float* t) {
    if (!c || !d || !t || n == 0 || transfer > VCT_TRANSFER_SRGB) return -1;
    if (hipSetDevice(c->device) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_transfer, dim3(blocks(n)), dim3(256), 0, c->stream, d, n, transfer, t);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" vct_status vct_luminance_meter_device(vct_ctx* c, const float* linear4, uint32_t w, uint32_t h, uint32_t* hist,
                                                 uint32_t* counts) {
    if (!c) return VCT_EINVAL;
    if (!linear4 || !hist || !counts) return lfail(c, VCT_EINVAL, "luminance_meter: NULL frame, hist or counts");
    if (((uintptr_t)linear4 & 15u) != 0 || (((uintptr_t)hist | (uintptr_t)counts) & 3u) != 0)
        return lfail(c, VCT_EINVAL, "luminance_meter: the frame must be 16-byte, hist and counts 4-byte aligned");
    if (!dims_ok(w, h)) return lfail(c, VCT_EINVAL, "luminance_meter: width or height outside 1 .. VCT_PRESENT_MAX_DIM");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    if ((e = hipMemsetAsync(hist, 0, kBins * sizeof(uint32_t), c->stream)) != hipSuccess) return lhip(c, e, "luminance_meter: clear hist");
    if ((e = hipMemsetAsync(counts, 0, 4 * sizeof(uint32_t), c->stream)) != hipSuccess) return lhip(c, e, "luminance_meter: clear counts");
    const uint32_t npx = w * h;             // <= 2^28
    const uint32_t want = (npx + kMeterThreads - 1) / kMeterThreads, nb = want < kMeterBlocks ? want : kMeterBlocks;
    if (g_meter_agg.load())
        hipLaunchKernelGGL(k_meter<true>, dim3(nb), dim3(kMeterThreads), 0, c->stream, (const float4*)linear4, npx, hist, counts);
    else
        hipLaunchKernelGGL(k_meter<false>, dim3(nb), dim3(kMeterThreads), 0, c->stream, (const float4*)linear4, npx, hist, counts);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "luminance_meter");
    return VCT_OK;
}

extern "C" vct_status vct_exposure_update_device(vct_ctx* c, const uint32_t* hist, const uint32_t* counts,
                                                 const vct_exposure_params* p, const vct_exposure_state* prev,
                                                 vct_exposure_state* out) {
    if (!c) return VCT_EINVAL;
    if (!hist || !counts || !p || !out) return lfail(c, VCT_EINVAL, "exposure_update: NULL hist, counts, params or out_state");
    if ((((uintptr_t)hist | (uintptr_t)counts | (uintptr_t)prev | (uintptr_t)out) & 3u) != 0)
        return lfail(c, VCT_EINVAL, "exposure_update: hist, counts and the records must be 4-byte aligned");
    if (!exposure_ok(p->key_value) || !exposure_ok(p->min_exposure) || !exposure_ok(p->max_exposure) ||
        !(p->min_exposure <= p->max_exposure))
        return lfail(c, VCT_EINVAL, "exposure_update: key_value, min_exposure <= max_exposure must be finite, > 0 and <= 2^64");
    if (p->low_permille >= 1000u || p->high_permille >= 1000u || p->low_permille + p->high_permille >= 1000u)
        return lfail(c, VCT_EINVAL, "exposure_update: low_permille + high_permille must be below 1000");
    if (!(p->rate_up >= 0.0f && p->rate_up <= 1.0f) || !(p->rate_down >= 0.0f && p->rate_down <= 1.0f))
        return lfail(c, VCT_EINVAL, "exposure_update: the rates must be in [0, 1]");
    if (p->reserved != 0) return lfail(c, VCT_EINVAL, "exposure_update: reserved != 0");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    ExposureK k;
    k.hist = hist; k.counts = counts; k.prev = prev; k.out = out; k.p = *p;
    hipLaunchKernelGGL(k_exposure, dim3(1), dim3(64), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "exposure_update");
    return VCT_OK;
}

extern "C" vct_status vct_bloom_scratch_bytes(uint32_t w, uint32_t h, uint32_t levels, size_t* bytes) {
    if (!bytes || !dims_ok(w, h) || levels < 1 || levels > VCT_BLOOM_MAX_LEVELS) return VCT_EINVAL;
    *bytes = bloom_levels(w, h, levels).texels * sizeof(float4);
    return VCT_OK;
}

extern "C" vct_status vct_bloom_device(vct_ctx* c, const float* linear4, uint32_t w, uint32_t h, const vct_bloom_params* p,
                                       const vct_exposure_state* state, float* scratch, size_t scratch_bytes) {
    if (!c) return VCT_EINVAL;
    if (!linear4 || !p || !scratch) return lfail(c, VCT_EINVAL, "bloom: NULL frame, params or scratch");
    if ((((uintptr_t)linear4 | (uintptr_t)scratch) & 15u) != 0 || ((uintptr_t)state & 3u) != 0)
        return lfail(c, VCT_EINVAL, "bloom: the frame and the scratch must be 16-byte, the record 4-byte aligned");
    if (!dims_ok(w, h)) return lfail(c, VCT_EINVAL, "bloom: width or height outside 1 .. VCT_PRESENT_MAX_DIM");
    if (p->levels < 1 || p->levels > VCT_BLOOM_MAX_LEVELS) return lfail(c, VCT_EINVAL, "bloom: levels outside 1 .. VCT_BLOOM_MAX_LEVELS");
    if (!(p->threshold >= 0.0f) || !std::isfinite(p->threshold)) return lfail(c, VCT_EINVAL, "bloom: threshold must be finite and >= 0");
    if (!state && !exposure_ok(p->exposure)) return lfail(c, VCT_EINVAL, "bloom: exposure must be finite, > 0 and <= 2^64");
    if (p->reserved != 0) return lfail(c, VCT_EINVAL, "bloom: reserved != 0");
    const BloomLevels L = bloom_levels(w, h, p->levels);
    if (scratch_bytes < L.texels * sizeof(float4)) return lfail(c, VCT_EINVAL, "bloom: scratch_bytes below vct_bloom_scratch_bytes");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    float4* s = (float4*)scratch;
    BloomPreK k;
    k.lin = (const float4*)linear4; k.state = state; k.out = s;
    k.w = (int)w; k.h = (int)h; k.ow = (int)L.w[0]; k.oh = (int)L.h[0];
    k.E = p->exposure; k.thr = p->threshold;
    hipLaunchKernelGGL(k_bloom_pre, dim3(blocks((size_t)L.w[0] * L.h[0])), dim3(256), 0, c->stream, k);
    for (uint32_t j = 1; j < L.n; ++j)
        hipLaunchKernelGGL(k_bloom_down, dim3(blocks((size_t)L.w[j] * L.h[j])), dim3(256), 0, c->stream, s + L.off[j - 1],
                           (int)L.w[j - 1], (int)L.h[j - 1], s + L.off[j], (int)L.w[j], (int)L.h[j]);
    for (uint32_t j = L.n - 1; j-- > 0;)
        hipLaunchKernelGGL(k_bloom_up, dim3(blocks((size_t)L.w[j] * L.h[j])), dim3(256), 0, c->stream, s + L.off[j], (int)L.w[j],
                           (int)L.h[j], s + L.off[j + 1], (int)L.w[j + 1], (int)L.h[j + 1]);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "bloom");
    return VCT_OK;
}

extern "C" vct_status vct_present_device(vct_ctx* c, const float* linear4, uint32_t w, uint32_t h, const vct_present_params* p,
                                         const vct_exposure_state* state, const float* bloom_half4, float* out_display4,
                                         uint32_t* out_rgba8) {
    if (!c) return VCT_EINVAL;
    if (!linear4 || !p) return lfail(c, VCT_EINVAL, "present: NULL frame or params");
    if (!out_display4 && !out_rgba8) return lfail(c, VCT_EINVAL, "present: no output");
    if ((((uintptr_t)linear4 | (uintptr_t)bloom_half4 | (uintptr_t)out_display4) & 15u) != 0 ||
        (((uintptr_t)state | (uintptr_t)out_rgba8) & 3u) != 0)
        return lfail(c, VCT_EINVAL, "present: float4 planes must be 16-byte, the record and out_rgba8 4-byte aligned");
    if (!dims_ok(w, h)) return lfail(c, VCT_EINVAL, "present: width or height outside 1 .. VCT_PRESENT_MAX_DIM");
    if (p->curve > VCT_CURVE_CLAMP || p->transfer > VCT_TRANSFER_SRGB || p->dither > 1u)
        return lfail(c, VCT_EINVAL, "present: unknown curve, transfer or dither");
    if (!state && !exposure_ok(p->exposure)) return lfail(c, VCT_EINVAL, "present: exposure must be finite, > 0 and <= 2^64");
    if (p->curve == VCT_CURVE_REINHARD_WHITE && !(p->white * p->white > 0.0f && std::isfinite(p->white * p->white)))
        return lfail(c, VCT_EINVAL, "present: white and white * white must be finite and > 0");
    if (bloom_half4 && !(p->bloom_intensity >= 0.0f && std::isfinite(p->bloom_intensity)))
        return lfail(c, VCT_EINVAL, "present: bloom_intensity must be finite and >= 0");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return lfail(c, VCT_EINVAL, "present: reserved != 0");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    PresentK k;
    k.lin = (const float4*)linear4; k.bloom = (const float4*)bloom_half4; k.state = state;
    k.disp = (float4*)out_display4; k.rgba8 = out_rgba8;
    k.npx = w * h; k.w = (int)w; k.bw = (int)((w + 1) / 2); k.bh = (int)((h + 1) / 2);
    k.E = p->exposure; k.white2 = p->white * p->white; k.intensity = p->bloom_intensity;
    k.curve = p->curve; k.transfer = p->transfer; k.dither = p->dither;
    if (bloom_half4 || p->dither) hipLaunchKernelGGL(k_present<true>, dim3(blocks(k.npx)), dim3(256), 0, c->stream, k);
    else hipLaunchKernelGGL(k_present<false>, dim3(blocks(k.npx)), dim3(256), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "present");
    return VCT_OK;
}
