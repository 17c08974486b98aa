// vct_mixed.hip — the mixed-resolution trace (include/vct_mixed.h; include/vct_spec.h
// "mixed-resolution trace").  K4 itself is untouched: a cone selection is a launch parameter
// (launch_trace), and K4's result for a pixel depends only on that pixel's record, so a low
// frame of picked records and a packed frame of hole records are traced by the same kernel.
//
//   kmix_pick     one lane per low pixel (8x8 low pixels per wave): the nearest valid pixel of
//                 its factor x factor block, records copied as float4.
//   kmix_up       one lane per full pixel (8x8 per wave): background / representative /
//                 blend / hole.  A wave's holes are one ballot: byte r of it is the hole mask
//                 of the wave's row r, stored at mask[y][x / 8] (rows padded to whole bytes, so
//                 the mask's bit order is row-major pixel order).  No atomics: one address
//                 counted into by every wave of a frame costs more than the whole kernel.
//   kmix_scan     one block: each row's holes from its mask bytes, their exclusive scan (holes
//                 before each row), the count and the stats.
//   kmix_list     one wave per row: hole k = holes before the row + set bits before the pixel
//                 (a wave scan over the row's mask bytes).  k < max_holes: the three records
//                 and the pixel index into the packed hole frame; the others get the fallback
//                 blend.  Extra waves clear the hole frame from min(count, max_holes) on.
//   kmix_scatter  plane[px[k]] = hole_plane[k], k < min(count, max_holes).
//
// A wave of kmix_up reads at most a 6x6 patch of low pixels at factor 2 (3x3 at factor 4): 36
// records of 52 bytes for 64 lanes x 4 taps.  The taps are left to the caches: the patch is
// reread by neighbouring waves only, the kernel holds no LDS and no barrier, and it is bound by
// its full-resolution reads and writes (DESIGN 10.7 has the resource table and the rate).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "vct_internal.h"
#include "vct_light_terms.h"

namespace vct {
namespace {

static_assert(sizeof(vct_mixed_params) == 16, "vct_mixed_params is 4 words (include/vct_mixed.h)");

constexpr uint32_t kNoSrc = VCT_MIXED_NO_SOURCE;
constexpr uint32_t kHoleW = VCT_MIXED_HOLE_WIDTH;
constexpr uint32_t kClearWaves = 256;    // waves of kmix_list that clear the hole frame's tail

struct PickK {
    const float4 *pos, *nrm, *alb;
    float4 *lpos, *lnrm, *lalb;
    uint32_t* lsrc;
    int w, h, wl, hl, f, tiles_x;
    float ex, ey, ez;
};

__global__ void __launch_bounds__(64) kmix_pick(const PickK k) {
    const int lane = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / k.tiles_x, tx = (int)blockIdx.x - ty * k.tiles_x;
    const int X = tx * 8 + (lane & 7), Y = ty * 8 + (lane >> 3);
    if (X >= k.wl || Y >= k.hl) return;
    uint32_t best = kNoSrc;
    float best_key = 0.0f;
    for (int j = 0; j < k.f; ++j) {
        const int y = Y * k.f + j;
        if (y >= k.h) break;
        for (int i = 0; i < k.f; ++i) {
            const int x = X * k.f + i;
            if (x >= k.w) break;
            const uint32_t p = (uint32_t)y * (uint32_t)k.w + (uint32_t)x;
            const float4 P = k.pos[p];
            if (!(P.w != 0.0f)) continue;
            const float dx = P.x - k.ex, dy = P.y - k.ey, dz = P.z - k.ez;
            float key = dot3(dx, dy, dz, dx, dy, dz);
            if (key != key) key = __builtin_inff();
            if (best == kNoSrc || key < best_key) { best = p; best_key = key; }
        }
    }
    const size_t q = (size_t)Y * (size_t)k.wl + (size_t)X;
    float4 rp = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rn = rp, ra = rp;
    if (best != kNoSrc) {
        rp = k.pos[best];
        rn = k.nrm[best];
        ra = k.alb[best];
    }
    k.lpos[q] = rp;
    k.lnrm[q] = rn;
    k.lalb[q] = ra;
    k.lsrc[q] = best;
}

struct UpK {
    const float4 *pos, *nrm, *alb;
    const float4 *lpos, *lnrm, *lplane;
    const uint32_t* lsrc;
    float4* plane;
    uint8_t* mask;           // [h][rowbytes], rowbytes = tiles_x rounded up to 16
    uint32_t* rowcnt;        // [h]: holes before the row (kmix_scan)
    uint32_t* wstat;         // [waves of kmix_up]: representatives | interpolated << 16 (with stats only)
    float4 *hpos, *hnrm, *halb;
    uint32_t* hpx;
    uint32_t* count;
    uint32_t* stats;
    uint32_t max_holes, hole_cap;   // hole_cap = 64 * rows of the hole frame
    int w, h, wl, hl, f, tiles_x, rowbytes;
    float ncos, eps;
};

// The blend of pixel (x, y), record P / N, over its four taps; tests: the normal and plane
// tests decide (false: the overflow fallback over every remaining tap).  -> W, S in `s`.
__device__ __forceinline__ uint32_t mix_blend(const UpK& k, int x, int y, const float4 P, const float4 N,
                                              bool tests, float4& s) {
    const int f2 = 2 * k.f;
    const int tx = 2 * x + 1 - k.f, ty = 2 * y + 1 - k.f;     // > -f2: the floor is -1 or the quotient
    const int X0 = tx < 0 ? -1 : tx / f2, Y0 = ty < 0 ? -1 : ty / f2;
    const int rx = tx - f2 * X0, ry = ty - f2 * Y0;
    uint32_t W = 0;
    s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i = t & 1, j = t >> 1;
        const int X = X0 + i, Y = Y0 + j;
        const int bw = (i ? rx : f2 - rx) * (j ? ry : f2 - ry);
        if (X < 0 || X >= k.wl || Y < 0 || Y >= k.hl || bw == 0) continue;
        const size_t q = (size_t)Y * (size_t)k.wl + (size_t)X;
        if (k.lsrc[q] == kNoSrc) continue;
        if (tests) {
            const float4 Nq = k.lnrm[q], Pq = k.lpos[q];
            const float c = dot3(N.x, N.y, N.z, Nq.x, Nq.y, Nq.z);
            const float d = fabsf(dot3(N.x, N.y, N.z, Pq.x - P.x, Pq.y - P.y, Pq.z - P.z));
            if (!(c >= k.ncos) || !(d <= k.eps)) continue;
        }
        const float4 V = k.lplane[q];
        const float fb = (float)bw;
        if (W == 0) s = make_float4(fb * V.x, fb * V.y, fb * V.z, fb * V.w);
        else { s.x = s.x + fb * V.x; s.y = s.y + fb * V.y; s.z = s.z + fb * V.z; s.w = s.w + fb * V.w; }
        W += (uint32_t)bw;
    }
    return W;
}

__global__ void __launch_bounds__(64) kmix_up(const UpK k) {
    const int lane = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / k.tiles_x, tx = (int)blockIdx.x - ty * k.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const bool inframe = x < k.w && y < k.h;
    const uint32_t i = inframe ? (uint32_t)y * (uint32_t)k.w + (uint32_t)x : 0u;
    float4 P = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inframe) P = k.pos[i];
    const bool valid = inframe && P.w != 0.0f;
    bool rep = false, hole = false;
    if (valid) {
        const size_t q = (size_t)(y / k.f) * (size_t)k.wl + (size_t)(x / k.f);
        if (k.lsrc[q] == i) {
            rep = true;
            k.plane[i] = k.lplane[q];
        } else {
            float4 s;
            const uint32_t W = mix_blend(k, x, y, P, k.nrm[i], true, s);
            if (W != 0) {
                const float fw = (float)W;
                k.plane[i] = make_float4(s.x / fw, s.y / fw, s.z / fw, s.w / fw);
            } else {
                hole = true;
            }
        }
    } else if (inframe) {
        k.plane[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const unsigned long long hb = __builtin_amdgcn_ballot_w64(hole);
    const unsigned long long rb = __builtin_amdgcn_ballot_w64(rep);
    const unsigned long long vb = __builtin_amdgcn_ballot_w64(valid);
    if (lane < 8) {
        const int row = ty * 8 + lane;
        if (row < k.h) {
            const uint32_t byte = (uint32_t)(hb >> (8 * lane)) & 0xffu;
            k.mask[(size_t)row * (size_t)k.rowbytes + (size_t)tx] = (uint8_t)byte;
        }
    }
    if (k.stats && lane == 0) {                  // no atomics: one word per wave, summed by kmix_scan
        const uint32_t nr = (uint32_t)__builtin_popcountll(rb);
        const uint32_t ni = (uint32_t)__builtin_popcountll(vb) - nr - (uint32_t)__builtin_popcountll(hb);
        k.wstat[blockIdx.x] = nr | ni << 16;
    }
}

// inclusive scan over the wave's lanes
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// one block: a thread counts a row's holes from its mask bytes (16 per load; the bytes past
// tiles_x are padding), the block scans the counts, and with stats sums kmix_up's wave words
__global__ void __launch_bounds__(1024) kmix_scan(const UpK k) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t srep[16], sint[16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < (uint32_t)k.h; base += 1024u) {
        const uint32_t r = base + (uint32_t)tid;
        uint32_t v = 0;
        if (r < (uint32_t)k.h) {
            const uint4* row = (const uint4*)(k.mask + (size_t)r * (size_t)k.rowbytes);
            for (int j = 0; j < k.rowbytes / 16; ++j) {
                const uint4 q = row[j];
                const uint32_t word[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int nb = k.tiles_x - (16 * j + 4 * c);   // bytes of this word inside the row
                    const uint32_t keep = nb >= 4 ? 0xffffffffu : (nb <= 0 ? 0u : (1u << (8 * nb)) - 1u);
                    v += (uint32_t)__builtin_popcount(word[c] & keep);
                }
            }
        }
        const uint32_t incl = wave_incl_scan(v, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t woff = 0, tot = 0;
        for (int j = 0; j < 16; ++j) {
            const uint32_t s = wsum[j];
            if (j < wave) woff += s;
            tot += s;
        }
        if (r < (uint32_t)k.h) k.rowcnt[r] = carry + woff + incl - v;
        carry += tot;
        __syncthreads();
    }
    uint32_t nr = 0, ni = 0;
    if (k.stats) {
        const uint32_t waves = (uint32_t)k.tiles_x * (uint32_t)((k.h + 7) / 8);
        for (uint32_t i = (uint32_t)tid; i < waves; i += 1024u) {
            const uint32_t ws = k.wstat[i];
            nr += ws & 0xffffu;
            ni += ws >> 16;
        }
        nr = wave_sum_u32(nr);
        ni = wave_sum_u32(ni);
        if (lane == 0) { srep[wave] = nr; sint[wave] = ni; }
        __syncthreads();
    }
    if (tid == 0) {
        *k.count = carry;
        if (k.stats) {
            nr = ni = 0;
            for (int j = 0; j < 16; ++j) { nr += srep[j]; ni += sint[j]; }
            k.stats[0] = nr;
            k.stats[1] = ni;
            k.stats[2] = carry;
            k.stats[3] = carry > k.max_holes ? carry - k.max_holes : 0u;
        }
    }
}

__global__ void __launch_bounds__(64) kmix_list(const UpK k) {
    const int lane = (int)threadIdx.x;
    if (blockIdx.x >= (uint32_t)k.h) {           // clear the hole frame from the last listed hole on
        const uint32_t cnt = *k.count;
        const uint32_t start = cnt < k.max_holes ? cnt : k.max_holes;
        const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (uint32_t e = start + (blockIdx.x - (uint32_t)k.h) * 64u + (uint32_t)lane; e < k.hole_cap; e += kClearWaves * 64u) {
            k.hpos[e] = z;
            k.hnrm[e] = z;
            k.halb[e] = z;
        }
        return;
    }
    const int y = (int)blockIdx.x;
    uint32_t carry = k.rowcnt[y];
    for (int base = 0; base < k.tiles_x; base += 64) {
        const int bx = base + lane;
        uint32_t byte = bx < k.tiles_x ? (uint32_t)k.mask[(size_t)y * (size_t)k.rowbytes + (size_t)bx] : 0u;
        const uint32_t n = (uint32_t)__builtin_popcount(byte);
        const uint32_t incl = wave_incl_scan(n, lane);
        uint32_t kk = carry + incl - n;
        carry += (uint32_t)__shfl(incl, 63, 64);
        while (byte) {
            const int b = __builtin_ctz(byte);
            byte &= byte - 1u;
            const int x = bx * 8 + b;
            if (x >= k.w) break;                 // kmix_up sets no such bit
            const uint32_t i = (uint32_t)y * (uint32_t)k.w + (uint32_t)x;
            const uint32_t kh = kk++;
            if (kh < k.max_holes) {
                k.hpos[kh] = k.pos[i];
                k.hnrm[kh] = k.nrm[i];
                k.halb[kh] = k.alb[i];
                k.hpx[kh] = i;
            } else {
                float4 s;
                const uint32_t W = mix_blend(k, x, y, k.pos[i], k.nrm[i], false, s);
                const float fw = (float)W;
                // W > 0: the pixel's own block is one of its taps and holds a valid pixel
                k.plane[i] = W ? make_float4(s.x / fw, s.y / fw, s.z / fw, s.w / fw) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
    }
}

__global__ void __launch_bounds__(256) kmix_scatter(const float4* __restrict__ hplane, const uint32_t* __restrict__ px,
                                                    const uint32_t* __restrict__ count, uint32_t max_holes,
                                                    float4* __restrict__ plane) {
    const uint32_t kh = blockIdx.x * 256u + threadIdx.x;
    const uint32_t cnt = *count;
    if (kh < (cnt < max_holes ? cnt : max_holes)) plane[px[kh]] = hplane[kh];
}

// ---- host side --------------------------------------------------------------------------
inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

const char* check_frame(uint32_t w, uint32_t h, uint32_t f) {
    if (f != 2 && f != 4) return "factor must be 2 or 4";
    if (w == 0 || h == 0 || w > 65536 || h > 65536 || (uint64_t)w * h > 0x7fffffffull) return "bad frame size";
    return nullptr;
}

// the params' input rule; *m = the capacity after the 0 -> ceil(w h / 8) rule
const char* check_params(const vct_mixed_params& p, uint32_t w, uint32_t h, uint32_t* m) {
    if (!std::isfinite(p.normal_cos) || p.normal_cos < -1.0f || p.normal_cos > 1.0f) return "normal_cos outside [-1, 1]";
    if (!std::isfinite(p.plane_eps) || std::signbit(p.plane_eps)) return "plane_eps not finite or negative";
    *m = p.max_holes ? p.max_holes : (uint32_t)(((uint64_t)w * h + 7u) / 8u);
    if (*m > kHoleW * 65536u) return "max_holes above 64 x 65536 (the hole frame's height limit)";
    return nullptr;
}

vct_status state_ok(vct_ctx* c, const char* what) {
    if (!c->grid.voxelized || !c->grid.mipped)
        return lfail(c, VCT_ESTATE, std::string(what) + " before voxelize / build_mips");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    return VCT_OK;
}

vct_status pick(vct_ctx* c, const float* pos4, const float* nrm4, const float* alb4, uint32_t w, uint32_t h,
                const float eye[3], uint32_t f, float* lp, float* ln, float* la, uint32_t* ls) {
    PickK k;
    k.pos = (const float4*)pos4; k.nrm = (const float4*)nrm4; k.alb = (const float4*)alb4;
    k.lpos = (float4*)lp; k.lnrm = (float4*)ln; k.lalb = (float4*)la; k.lsrc = ls;
    k.w = (int)w; k.h = (int)h; k.f = (int)f;
    k.wl = (int)((w + f - 1) / f); k.hl = (int)((h + f - 1) / f);
    k.tiles_x = (k.wl + 7) / 8;
    k.ex = eye[0]; k.ey = eye[1]; k.ez = eye[2];
    hipLaunchKernelGGL(kmix_pick, dim3((uint32_t)k.tiles_x * (uint32_t)((k.hl + 7) / 8)), dim3(64), 0, c->stream, k);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? VCT_OK : lhip(c, e, "mixed_pick");
}

// m: the resolved capacity (== holes.max_holes)
vct_status upsample(vct_ctx* c, const float* pos4, const float* nrm4, const float* alb4, uint32_t w, uint32_t h,
                    uint32_t f, const float* lp, const float* ln, const uint32_t* ls, const float* lplane,
                    const vct_mixed_params& p, uint32_t m, float* plane4, const vct_mixed_holes& ho) {
    UpK k;
    std::memset(&k, 0, sizeof k);
    k.pos = (const float4*)pos4; k.nrm = (const float4*)nrm4; k.alb = (const float4*)alb4;
    k.lpos = (const float4*)lp; k.lnrm = (const float4*)ln; k.lplane = (const float4*)lplane; k.lsrc = ls;
    k.plane = (float4*)plane4;
    k.w = (int)w; k.h = (int)h; k.f = (int)f;
    k.wl = (int)((w + f - 1) / f); k.hl = (int)((h + f - 1) / f);
    k.tiles_x = (int)((w + 7) / 8);
    k.ncos = p.normal_cos; k.eps = p.plane_eps;
    k.hpos = (float4*)ho.pos4; k.hnrm = (float4*)ho.nrm4; k.halb = (float4*)ho.alb4;
    k.hpx = ho.px; k.count = ho.count; k.stats = ho.stats;
    k.max_holes = m;
    k.hole_cap = ((m + kHoleW - 1) / kHoleW) * kHoleW;
    k.rowbytes = (k.tiles_x + 15) & ~15;
    // scratch of the stream: [rowcnt h | wstat waves | mask h x rowbytes]; every word read is
    // written by the launch before it, so nothing is cleared
    const uint32_t waves = (uint32_t)k.tiles_x * ((h + 7) / 8);
    const size_t cnt_bytes = al256((size_t)h * 4), ws_bytes = al256((size_t)waves * 4);
    void* sp = nullptr;
    hipError_t e = k4_scratch(c, kScMixUp, cnt_bytes + ws_bytes + (size_t)h * (size_t)k.rowbytes, &sp, nullptr);
    if (e != hipSuccess) return lhip(c, e, "mixed_upsample: scratch");
    k.rowcnt = (uint32_t*)sp;
    k.wstat = (uint32_t*)((char*)sp + cnt_bytes);
    k.mask = (uint8_t*)sp + cnt_bytes + ws_bytes;
    hipLaunchKernelGGL(kmix_up, dim3(waves), dim3(64), 0, c->stream, k);
    hipLaunchKernelGGL(kmix_scan, dim3(1), dim3(1024), 0, c->stream, k);
    hipLaunchKernelGGL(kmix_list, dim3(h + kClearWaves), dim3(64), 0, c->stream, k);
    e = hipGetLastError();
    return e == hipSuccess ? VCT_OK : lhip(c, e, "mixed_upsample");
}

vct_status scatter(vct_ctx* c, const float* hplane, const vct_mixed_holes& ho, float* plane4) {
    hipLaunchKernelGGL(kmix_scatter, dim3((ho.max_holes + 255u) / 256u), dim3(256), 0, c->stream, (const float4*)hplane,
                       (const uint32_t*)ho.px, (const uint32_t*)ho.count, ho.max_holes, (float4*)plane4);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? VCT_OK : lhip(c, e, "mixed_scatter");
}

// vct_trace_device's argument rule, with an unselected plane pointer free to be NULL
const char* check_trace_args(const vct_trace_args* a, uint32_t cones) {
    if (!a->pos4 || !a->nrm4 || !a->alb4) return "null G-buffer pointer";
    if (((cones & VCT_CONES_DIFFUSE) && !a->diffuse4) || ((cones & VCT_CONES_SPECULAR) && !a->spec4))
        return "null output pointer";
    if (a->width == 0 || a->height == 0 || a->width > 65536 || a->height > 65536 ||
        (uint64_t)a->width * a->height > 0xffffffffull)
        return "bad frame size";
    if (a->tile_world > 1 && a->tile_rank >= a->tile_world) return "tile_rank >= tile_world";
    if (((uintptr_t)a->cone_steps & 7) || ((uintptr_t)a->texel_fetches & 7))
        return "cone_steps / texel_fetches must be 8-byte aligned";
    if (!al16(a->pos4) || !al16(a->nrm4) || !al16(a->alb4) || !al16(a->diffuse4) || !al16(a->spec4))
        return "G-buffer / output pointers must be 16-byte aligned";
    return nullptr;
}

// pixels of the plane a launch of `a` writes (the rank-compact layout counts whole tiles)
size_t plane_pixels(const vct_trace_args* a) {
    if (!a->tile_compact) return (size_t)a->width * a->height;
    return (size_t)tiles_for_rank(a->width, a->height, a->tile_world ? a->tile_rank : 0, a->tile_world ? a->tile_world : 1) *
           VCT_TILE * VCT_TILE;
}

// one cone set (cones = 1 or 2) of `a`, checked already; on this context's device
vct_status trace_sel(vct_ctx* c, const vct_trace_args* a, uint32_t cones, const char* what) {
    const bool diff = cones == VCT_CONES_DIFFUSE;
    hipError_t e;
    if (diff ? c->cfg.n_diffuse == 0 : c->cfg.specular == 0) {    // cones the context lacks: +0, no steps
        if ((e = hipMemsetAsync(diff ? a->diffuse4 : a->spec4, 0, plane_pixels(a) * 16, c->stream)) != hipSuccess)
            return lhip(c, e, what);
        if (a->steps_px && (e = hipMemsetAsync(a->steps_px, 0, (size_t)a->width * a->height * 4, c->stream)) != hipSuccess)
            return lhip(c, e, what);
        return VCT_OK;
    }
    // K4 writes both planes: the other one goes to scratch of the stream
    void* un = nullptr;
    if ((e = k4_scratch(c, kScUnsel, plane_pixels(a) * 16, &un, nullptr)) != hipSuccess) return lhip(c, e, what);
    vct_trace_args b = *a;
    if (diff) b.spec4 = (float*)un;
    else b.diffuse4 = (float*)un;
    if ((e = launch_trace(c, &b, -1, cones)) != hipSuccess) return lhip(c, e, what);
    return VCT_OK;
}

}  // namespace
}  // namespace vct

using namespace vct;

extern "C" vct_status vct_mixed_default_params(const vct_ctx* c, uint32_t factor, vct_mixed_params* out) {
    if (!c || !out || (factor != 2 && factor != 4)) return VCT_EINVAL;
    out->normal_cos = VCT_MIXED_NORMAL_COS;
    out->plane_eps = (float)factor * (c->cfg.extent / (float)c->cfg.n);
    out->max_holes = 0;
    out->factor = factor;
    return VCT_OK;
}

extern "C" vct_status vct_trace_cones_device(vct_ctx* c, const vct_trace_args* a, uint32_t cones) {
    if (!c || !a) return VCT_EINVAL;
    if (cones == 0 || cones > 3) return lfail(c, VCT_EINVAL, "trace_cones: cones must be VCT_CONES_DIFFUSE, _SPECULAR or both");
    if (cones == 3) return vct_trace_device(c, a);
    if (!c->grid.mipped) return lfail(c, VCT_ESTATE, "trace_cones before build_mips");
    if (const char* bad = check_trace_args(a, cones)) return lfail(c, VCT_EINVAL, std::string("trace_cones: ") + bad);
    vct_status st = state_ok(c, "trace_cones");
    if (st != VCT_OK) return st;
    return trace_sel(c, a, cones, "trace_cones");
}

extern "C" vct_status vct_mixed_pick_device(vct_ctx* c, const float* pos4, const float* nrm4, const float* alb4, uint32_t w,
                                            uint32_t h, const float eye[3], uint32_t factor, float* lo_pos4,
                                            float* lo_nrm4, float* lo_alb4, uint32_t* lo_src) {
    if (!c) return VCT_EINVAL;
    if (!pos4 || !nrm4 || !alb4 || !eye || !lo_pos4 || !lo_nrm4 || !lo_alb4 || !lo_src)
        return lfail(c, VCT_EINVAL, "mixed_pick: NULL buffer");
    if (const char* bad = check_frame(w, h, factor)) return lfail(c, VCT_EINVAL, std::string("mixed_pick: ") + bad);
    if (!al16(pos4) || !al16(nrm4) || !al16(alb4) || !al16(lo_pos4) || !al16(lo_nrm4) || !al16(lo_alb4) ||
        ((uintptr_t)lo_src & 3u))
        return lfail(c, VCT_EINVAL, "mixed_pick: float4 buffers must be 16-byte aligned");
    vct_status st = state_ok(c, "mixed_pick");
    if (st != VCT_OK) return st;
    return pick(c, pos4, nrm4, alb4, w, h, eye, factor, lo_pos4, lo_nrm4, lo_alb4, lo_src);
}

extern "C" vct_status vct_mixed_upsample_device(vct_ctx* c, const float* pos4, const float* nrm4, const float* alb4,
                                                uint32_t w, uint32_t h, uint32_t factor, const float* lo_pos4,
                                                const float* lo_nrm4, const uint32_t* lo_src, const float* lo_plane4,
                                                const vct_mixed_params* p, float* plane4, const vct_mixed_holes* ho) {
    if (!c) return VCT_EINVAL;
    if (!pos4 || !nrm4 || !alb4 || !lo_pos4 || !lo_nrm4 || !lo_src || !lo_plane4 || !p || !plane4 || !ho)
        return lfail(c, VCT_EINVAL, "mixed_upsample: NULL buffer");
    if (!ho->pos4 || !ho->nrm4 || !ho->alb4 || !ho->px || !ho->count)
        return lfail(c, VCT_EINVAL, "mixed_upsample: NULL hole buffer");
    if (const char* bad = check_frame(w, h, factor)) return lfail(c, VCT_EINVAL, std::string("mixed_upsample: ") + bad);
    uint32_t m = 0;
    if (const char* bad = check_params(*p, w, h, &m)) return lfail(c, VCT_EINVAL, std::string("mixed_upsample: ") + bad);
    if (ho->max_holes != m) return lfail(c, VCT_EINVAL, "mixed_upsample: holes->max_holes is not the params' capacity");
    if (!al16(pos4) || !al16(nrm4) || !al16(alb4) || !al16(lo_pos4) || !al16(lo_nrm4) || !al16(lo_plane4) ||
        !al16(plane4) || !al16(ho->pos4) || !al16(ho->nrm4) || !al16(ho->alb4))
        return lfail(c, VCT_EINVAL, "mixed_upsample: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)lo_src | (uintptr_t)ho->px | (uintptr_t)ho->count | (uintptr_t)ho->stats) & 3u)
        return lfail(c, VCT_EINVAL, "mixed_upsample: uint32 buffers must be 4-byte aligned");
    vct_status st = state_ok(c, "mixed_upsample");
    if (st != VCT_OK) return st;
    return upsample(c, pos4, nrm4, alb4, w, h, factor, lo_pos4, lo_nrm4, lo_src, lo_plane4, *p, m, plane4, *ho);
}

extern "C" vct_status vct_mixed_scatter_device(vct_ctx* c, const float* hole_plane4, const vct_mixed_holes* ho,
                                               float* plane4) {
    if (!c) return VCT_EINVAL;
    if (!hole_plane4 || !ho || !plane4 || !ho->px || !ho->count) return lfail(c, VCT_EINVAL, "mixed_scatter: NULL buffer");
    if (ho->max_holes == 0) return lfail(c, VCT_EINVAL, "mixed_scatter: holes->max_holes is 0");
    if (!al16(hole_plane4) || !al16(plane4) || (((uintptr_t)ho->px | (uintptr_t)ho->count) & 3u))
        return lfail(c, VCT_EINVAL, "mixed_scatter: misaligned buffer");
    vct_status st = state_ok(c, "mixed_scatter");
    if (st != VCT_OK) return st;
    return scatter(c, hole_plane4, *ho, plane4);
}

extern "C" vct_status vct_trace_mixed_device(vct_ctx* c, const vct_trace_args* a, const vct_mixed_params* p) {
    if (!c || !a || !p) return VCT_EINVAL;
    if (const char* bad = check_trace_args(a, 3)) return lfail(c, VCT_EINVAL, std::string("trace_mixed: ") + bad);
    if (a->steps_px) return lfail(c, VCT_EINVAL, "trace_mixed: steps_px must be NULL");
    if (a->tile_world > 1 || a->tile_compact) return lfail(c, VCT_EINVAL, "trace_mixed: tile_world / tile_compact must be 0");
    const uint32_t w = a->width, h = a->height, f = p->factor;
    if (const char* bad = check_frame(w, h, f)) return lfail(c, VCT_EINVAL, std::string("trace_mixed: ") + bad);
    uint32_t m = 0;
    if (const char* bad = check_params(*p, w, h, &m)) return lfail(c, VCT_EINVAL, std::string("trace_mixed: ") + bad);
    vct_status st = state_ok(c, "trace_mixed");
    if (st != VCT_OK) return st;
    const uint32_t wl = (w + f - 1) / f, hl = (h + f - 1) / f, rows = (m + kHoleW - 1) / kHoleW;
    const size_t lb = al256((size_t)wl * hl * 16), hb = al256((size_t)rows * kHoleW * 16);
    hipError_t e;
    void* un = nullptr;   // the largest launch's unselected plane first: the slot never grows inside the frame
    const size_t un_px = std::max((size_t)w * h, (size_t)rows * kHoleW);
    if ((e = k4_scratch(c, kScUnsel, un_px * 16, &un, nullptr)) != hipSuccess) return lhip(c, e, "trace_mixed: scratch");
    void* sp = nullptr;
    if ((e = k4_scratch(c, kScMixed, 5 * lb + 4 * hb + al256((size_t)m * 4) + 256, &sp, nullptr)) != hipSuccess)
        return lhip(c, e, "trace_mixed: scratch");
    char* b = (char*)sp;
    float* lpos = (float*)b; float* lnrm = (float*)(b + lb); float* lalb = (float*)(b + 2 * lb);
    float* ldif = (float*)(b + 3 * lb);
    uint32_t* lsrc = (uint32_t*)(b + 4 * lb);
    b += 5 * lb;
    vct_mixed_holes ho;
    ho.pos4 = (float*)b; ho.nrm4 = (float*)(b + hb); ho.alb4 = (float*)(b + 2 * hb);
    float* hdif = (float*)(b + 3 * hb);
    ho.px = (uint32_t*)(b + 4 * hb);
    ho.count = (uint32_t*)(b + 4 * hb + al256((size_t)m * 4));
    ho.stats = nullptr;
    ho.max_holes = m;
    if ((st = pick(c, a->pos4, a->nrm4, a->alb4, w, h, a->eye, f, lpos, lnrm, lalb, lsrc)) != VCT_OK) return st;
    vct_trace_args t = *a;
    t.pos4 = lpos; t.nrm4 = lnrm; t.alb4 = lalb; t.width = wl; t.height = hl; t.diffuse4 = ldif; t.spec4 = nullptr;
    if ((st = trace_sel(c, &t, VCT_CONES_DIFFUSE, "trace_mixed: low frame")) != VCT_OK) return st;
    if ((st = upsample(c, a->pos4, a->nrm4, a->alb4, w, h, f, lpos, lnrm, lsrc, ldif, *p, m, a->diffuse4, ho)) != VCT_OK)
        return st;
    t.pos4 = ho.pos4; t.nrm4 = ho.nrm4; t.alb4 = ho.alb4; t.width = kHoleW; t.height = rows; t.diffuse4 = hdif;
    if ((st = trace_sel(c, &t, VCT_CONES_DIFFUSE, "trace_mixed: hole frame")) != VCT_OK) return st;
    if ((st = scatter(c, hdif, ho, a->diffuse4)) != VCT_OK) return st;
    return trace_sel(c, a, VCT_CONES_SPECULAR, "trace_mixed: specular");
}
