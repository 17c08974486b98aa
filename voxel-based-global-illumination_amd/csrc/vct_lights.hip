// vct_lights.hip — K2 and the composite for a list of directional, point and spot lights
// (include/vct_lights.h; the arithmetic is include/vct_spec.h "local lights").
//
// A local light's work per voxel is uneven: a voxel may be out of range, outside the
// cone or facing away, and every walk has its own direction and its own end.  So the
// lights are not looped over inside the walking lane.  Per batch of up to 32 lights:
//   kl_pairs   one lane per (occupied-list entry, light), the light uniform per block
//              (its constants are scalar loads): the skip tests of the spec; a pair that
//              needs a shadow walk is appended to the pair list (ballot + mbcnt slots, one
//              atomic per 256 lanes; the order of the list is free);
//   kl_walk    one lane per pair: the walk of k2_walk (coarse occupancy bits in LDS, fine
//              words through a buffer resource, batched and branch-free) with per-lane
//              step signs and t increments, and the spec's second end (t_e >= t_lim);
//              an unblocked pair sets its light's bit in the voxel's 32-bit mask
//              (integer atomicOr: no float is ever added out of order);
//   kl_sum     one lane per occupied voxel: every light's unshadowed term again (the same
//              operations, so the same bits), times the mask bit, added in list order.
// The first batch writes level 0, later ones add to it.  The plain form (one light per
// pass: pairs -> walk -> sum with a batch of one) is the A/B baseline, vct_debug_lights.
//
// The composite of a light list is one kernel, kl_composite<VIS, EM>, behind three entry
// points: vct_composite_lights_device here (V walked), vct_composite_shadowed_device
// (vct_shadow.hip: V read from a vis plane) and vct_composite_emissive_device (vct_emission.hip:
// either, plus the emission term).  composite_light_list has the checks they share.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "vct_internal.h"
#include "vct_light_terms.h"

namespace vct {
namespace {

constexpr int kBatch = 32;                 // lights per batch: one bit each in a voxel's mask
constexpr int kCoarseRows = 64 * 64;       // k2_coarse's table: 64-bit rows, 32 KiB of LDS

struct LightBatch {
    DLight l[kBatch];
};

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The same V with the coarse bits (LDS) in front of the fine words, in batches of kB
// cells, as dda_coarse (vct_voxelize.hip) does for the uniform light direction: here the
// step signs and t increments are the lane's own.  A cell counts only while the walk is
// inside the grid and t_e < t_lim; both conditions, once false, stay false (every axis
// moves one way, t_e never decreases), so stepping a batch past either end is harmless.
// COUNT: *cells receives the cells the spec's walk tests.
template <int kB, bool COUNT>
__device__ __forceinline__ float dda_coarse_lim(__amdgpu_buffer_rsrc_t bits, const unsigned long long* __restrict__ cb,
                                                int lgn, int cs, int lgcn, float qx, float qy, float qz, float lx,
                                                float ly, float lz, float t_lim, uint32_t* cells) {
    const uint32_t N = 1u << lgn;
    int vx = (int)floorf(qx), vy = (int)floorf(qy), vz = (int)floorf(qz);
    if (max(max((uint32_t)vx, (uint32_t)vy), (uint32_t)vz) >= N) return 1.0f;
    const int sx = lx > 0.0f ? 1 : (lx < 0.0f ? -1 : 0);
    const int sy = ly > 0.0f ? 1 : (ly < 0.0f ? -1 : 0);
    const int sz = lz > 0.0f ? 1 : (lz < 0.0f ? -1 : 0);
    const float inf = __builtin_inff();
    const float tdx = sx ? 1.0f / fabsf(lx) : inf;
    const float tdy = sy ? 1.0f / fabsf(ly) : inf;
    const float tdz = sz ? 1.0f / fabsf(lz) : inf;
    float tmx = sx > 0 ? ((float)(vx + 1) - qx) * tdx : (sx < 0 ? (qx - (float)vx) * tdx : inf);
    float tmy = sy > 0 ? ((float)(vy + 1) - qy) * tdy : (sy < 0 ? (qy - (float)vy) * tdy : inf);
    float tmz = sz > 0 ? ((float)(vz + 1) - qz) * tdz : (sz < 0 ? (qz - (float)vz) * tdz : inf);
    float te = 0.0f;
    for (;;) {
        uint32_t cv[kB], co = 0u, vm = 0u;
#pragma unroll
        for (int b = 0; b < kB; ++b) {
            const uint32_t ux = (uint32_t)vx, uy = (uint32_t)vy, uz = (uint32_t)vz;
            const bool valid = (max(max(ux, uy), uz) < N) & (te < t_lim);
            cv[b] = ux | (uy << lgn) | (uz << (2 * lgn));
            // unconditional LDS read (an outside cell's row wrapped into the table; its bit is dropped)
            const unsigned long long row = cb[((uy >> cs) | ((uz >> cs) << lgcn)) & (uint32_t)(kCoarseRows - 1)];
            co |= ((uint32_t)(row >> ((ux >> cs) & 63u)) & (uint32_t)valid) << b;
            if (COUNT) vm |= (uint32_t)valid << b;
            // the spec's choice (x if tmx <= tmy, tmz; else y if tmy <= tmz; else z) from the
            // minimum, as dda_coarse has it: an axis whose td is +inf (K2 input rule) has a tm of
            // +inf or NaN and is never the minimum, so tmin is the chosen axis's t, never NaN
            const float tmin = fminf(fminf(tmx, tmy), tmz);
            const bool bx = tmx == tmin;
            const bool by = !bx && tmy == tmin;
            const bool bz = !bx && !by;
            const float nx = tmx + tdx, ny = tmy + tdy, nz = tmz + tdz;
            vx += bx ? sx : 0;
            vy += by ? sy : 0;
            vz += bz ? sz : 0;
            tmx = bx ? nx : tmx;
            tmy = by ? ny : tmy;
            tmz = bz ? nz : tmz;
            te = tmin;
        }
        // fine words only when some lane of the wave met a coarse-occupied cell; a cell
        // whose coarse bit is clear reads past the buffer (0)
        if (__builtin_amdgcn_ballot_w64(co != 0u)) {
            uint32_t hit = 0u;
#pragma unroll
            for (int b = 0; b < kB; ++b) {
                const uint32_t off = (co >> b) & 1u ? (cv[b] >> 6) << 3 : 0x80000000u;
                const auto w = __builtin_amdgcn_raw_buffer_load_b64(bits, off, 0, 0);
                const unsigned long long wd = ((unsigned long long)w[1] << 32) | w[0];
                if (COUNT) hit |= ((uint32_t)(wd >> (cv[b] & 63u)) & 1u) << b;
                else hit |= (uint32_t)(wd >> (cv[b] & 63u));
            }
            if (COUNT) {
                if (hit) { *cells += (uint32_t)__builtin_ctz(hit) + 1u; return 0.0f; }
            } else if (hit & 1u) {
                return 0.0f;
            }
        }
        if (COUNT) *cells += (uint32_t)__popc(vm);
        if (max(max((uint32_t)vx, (uint32_t)vy), (uint32_t)vz) >= N || te >= t_lim) return 1.0f;
    }
}

// k2_coarse's table (vct_voxelize.hip), for a first K2 after K1 that is a light list: bit bx
// of 64-bit row (by, bz) is set when any voxel of the brick (edge 2^cs) is occupied
__global__ void __launch_bounds__(256) kl_coarse(const unsigned long long* __restrict__ bits, int n, int cs,
                                                 uint32_t* __restrict__ coarse) {
    const int cn = n >> cs;
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;   // bit c = bx + 64 (by + cn bz)
    const uint32_t ncb = 64u * (uint32_t)cn * cn;
    bool any = false;
    if (c < ncb && (int)(c & 63u) < cn) {
        const int bx = (int)(c & 63u), by = (int)((c >> 6) % cn), bz = (int)((c >> 6) / cn);
        const int e = 1 << cs;
        for (int z = bz * e; z < bz * e + e && !any; ++z)
            for (int y = by * e; y < by * e + e && !any; ++y)
                for (int x = bx * e; x < bx * e + e; x += 64 < e ? 64 : e) {
                    const size_t v = (size_t)x + (size_t)n * ((size_t)y + (size_t)n * (size_t)z);
                    const int len = e < 64 ? e : 64;
                    const unsigned long long m = len == 64 ? ~0ull : ((1ull << len) - 1ull) << (v & 63);
                    if (bits[v >> 6] & m) { any = true; break; }
                }
    }
    const unsigned long long b = __ballot(any);
    if (c < ncb && (c & 31) == 0) coarse[c >> 5] = (uint32_t)(b >> (threadIdx.x & 32));
}

struct Receiver {
    uint32_t v;
    float qx, qy, qz, nx, ny, nz;
};

__device__ __forceinline__ Receiver receiver(uint32_t v, const float4* __restrict__ normal, int lgn) {
    const uint32_t m = (1u << lgn) - 1u;
    const float4 nm = normal[v];
    Receiver r;
    r.v = v;
    r.nx = nm.x; r.ny = nm.y; r.nz = nm.z;
    r.qx = ((float)(int)(v & m) + 0.5f) + nm.x;
    r.qy = ((float)(int)((v >> lgn) & m) + 0.5f) + nm.y;
    r.qz = ((float)(int)(v >> (2 * lgn)) + 0.5f) + nm.z;
    return r;
}

// blockIdx.y = the light of the batch; pair = (occupied-list index << lb) | light.  A pair
// past the list's capacity is walked here, plainly: the list is bounded whatever the scene.
__global__ void __launch_bounds__(256) kl_pairs(const uint32_t* __restrict__ occ, const uint32_t* __restrict__ n_occ,
                                                const float4* __restrict__ normal,
                                                const unsigned long long* __restrict__ bits, int lgn,
                                                const LightBatch batch, float h2, uint32_t lb,
                                                uint32_t* __restrict__ pairs, uint32_t* __restrict__ n_pairs,
                                                uint32_t cap, uint32_t* __restrict__ mask) {
    __shared__ uint32_t s_cnt[4];
    __shared__ uint32_t s_base;
    const uint32_t cnt = *n_occ;
    const uint32_t j = blockIdx.y;
    const DLight& L = batch.l[j];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t c0 = blockIdx.x * 256u; c0 < cnt; c0 += gridDim.x * 256u) {
        const uint32_t i = c0 + threadIdx.x;
        bool need = false;
        float lx = 0.0f, ly = 0.0f, lz = 0.0f, f, ndl, t_lim = 0.0f;
        Receiver r{};
        if (i < cnt) {
            r = receiver(occ[i], normal, lgn);
            need = light_terms(L, h2, r.qx, r.qy, r.qz, r.nx, r.ny, r.nz, lx, ly, lz, f, ndl, t_lim);
        }
        const unsigned long long b = __ballot(need);
        if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t run = 0;
            for (int q = 0; q < 4; ++q) {
                const uint32_t t = s_cnt[q];
                s_cnt[q] = run;
                run += t;
            }
            s_base = run ? atomicAdd(n_pairs, run) : 0u;
        }
        __syncthreads();
        if (need) {
            const uint32_t slot = s_base + s_cnt[wave] + lanes_below(b);
            if (slot < cap) {
                pairs[slot] = (i << lb) | j;
            } else if (dda_lim(bits, 1 << lgn, r.qx, r.qy, r.qz, lx, ly, lz, t_lim) != 0.0f) {
                atomicOr(&mask[i], 1u << j);
            }
        }
        __syncthreads();
    }
}

// one lane per pair; BS-thread blocks share one LDS copy of the coarse bits; KB cells per
// lookup batch (k2_walk's launch shape)
template <int KB, int BS, bool COUNT>
__global__ void __launch_bounds__(BS) kl_walk(const uint32_t* __restrict__ pairs, const uint32_t* __restrict__ n_pairs,
                                              uint32_t cap, uint32_t lb, const uint32_t* __restrict__ occ,
                                              const uint32_t* __restrict__ coarse, int cs,
                                              const float4* __restrict__ normal,
                                              const unsigned long long* __restrict__ bits, int lgn,
                                              const LightBatch batch, float h2, uint32_t* __restrict__ mask,
                                              unsigned long long* __restrict__ cells_total) {
    __shared__ unsigned long long cbits[kCoarseRows];
    const uint32_t cnt = min(*n_pairs, cap);
    if (blockIdx.x * BS >= cnt) return;           // block-uniform: no pair for this block
    const int lgcn = lgn - cs;
    const uint32_t nrow = 1u << (2 * lgcn);
    const unsigned long long* crow = reinterpret_cast<const unsigned long long*>(coarse);
    for (uint32_t i = threadIdx.x; i < nrow; i += BS) cbits[i] = crow[i];
    __syncthreads();
    const __amdgpu_buffer_rsrc_t br =
        __builtin_amdgcn_make_buffer_rsrc((void*)bits, (short)0, (int)(((size_t)1 << (3 * lgn)) >> 3), 0x00020000);
    uint32_t cells = 0;
    for (uint32_t p = blockIdx.x * BS + threadIdx.x; p < cnt; p += gridDim.x * BS) {
        const uint32_t pr = pairs[p];
        const uint32_t i = pr >> lb, j = pr & ((1u << lb) - 1u);
        const Receiver r = receiver(occ[i], normal, lgn);
        float lx, ly, lz, f, ndl, t_lim;
        // kl_pairs' terms again: the same operations on the same inputs, so the same l and t_lim
        if (!light_terms(batch.l[j], h2, r.qx, r.qy, r.qz, r.nx, r.ny, r.nz, lx, ly, lz, f, ndl, t_lim)) continue;
        const float vis = dda_coarse_lim<KB, COUNT>(br, cbits, lgn, cs, lgcn, r.qx, r.qy, r.qz, lx, ly, lz, t_lim, &cells);
        if (vis != 0.0f) atomicOr(&mask[i], 1u << j);
    }
    if (COUNT) {
        const uint32_t w = wave_sum_u32(cells);
        if ((threadIdx.x & 63) == 0 && w) atomicAdd(cells_total, (unsigned long long)w);
    }
}

// one lane per occupied voxel: the batch's lights in list order; clears the voxel's mask
// for the next batch
__global__ void __launch_bounds__(256) kl_sum(const uint32_t* __restrict__ occ, const uint32_t* __restrict__ n_occ,
                                              const float4* __restrict__ albedo_occ, const float4* __restrict__ normal,
                                              int lgn, const LightBatch batch, uint32_t nb, float h2, int first,
                                              uint32_t* __restrict__ mask, uint32_t* __restrict__ counters,
                                              float4* __restrict__ r0) {
    const uint32_t cnt = *n_occ;
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[1] += counters[0];   // pairs of the whole call (tools)
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < cnt; i += gridDim.x * 256u) {
        const Receiver r = receiver(occ[i], normal, lgn);
        const float4 ao = albedo_occ[r.v];
        const uint32_t m = mask[i];
        if (m) mask[i] = 0u;
        float4* const dst = r0 + l0_texel(r.v, 1u << lgn);
        float ar = 0.0f, ag = 0.0f, ab = 0.0f;
        if (!first) {
            const float4 old = *dst;
            ar = old.x; ag = old.y; ab = old.z;
        }
        for (uint32_t j = 0; j < nb; ++j) {
            const DLight& L = batch.l[j];
            float lx, ly, lz, f, ndl, t_lim;
            if (!light_terms(L, h2, r.qx, r.qy, r.qz, r.nx, r.ny, r.nz, lx, ly, lz, f, ndl, t_lim)) continue;
            const float vis = (m >> j) & 1u ? 1.0f : 0.0f;
            ar = ar + (((ao.x * L.cr) * ndl) * f) * vis;
            ag = ag + (((ao.y * L.cg) * ndl) * f) * vis;
            ab = ab + (((ao.z * L.cb) * ndl) * f) * vis;
        }
        *dst = make_float4(ar, ag, ab, 1.0f);
    }
}

// ---- composite + present for a light list (k_composite, vct_frame.hip, with the direct
// term of the spec): one lane per pixel, the lights in list order ---------------------------
struct CompK {
    const float4 *pos, *nrm, *alb, *diff, *spec;
    const float* vis;                      // VIS: [n_lights][h][w]
    const unsigned long long* bits;        // !VIS: K1's occupancy, for the walk
    const unsigned long long* em_bits;     // EM: the emission grid (Emission, vct_internal.h)
    const uint32_t* em_prefix;
    const float4* em_E;
    int n, w, h;
    float g0x, g0y, g0z, inv_h, h2, scale;
    uint32_t n_lights;
    float4* lin;
    uint32_t* rgba8;
};

// VIS: V read from the vis plane (vct_composite_shadowed_device), else the plain walk; EM: the
// grid may hold an emissive voxel and scale != 0 (vct_composite_emissive_device; without it,
// the arithmetic of the other two, unchanged)
template <bool VIS, bool EM>
__global__ void __launch_bounds__(256) kl_composite(const CompK k, const LightSet set) {
    const uint32_t npx = (uint32_t)k.w * (uint32_t)k.h;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npx) return;
    const float4 P = k.pos[i];
    if (P.w == 0.0f) {   // background: the reference's clear colour
        if (k.lin) k.lin[i] = make_float4(VCT_CLEAR_R, VCT_CLEAR_G, VCT_CLEAR_B, 0.0f);
        if (k.rgba8)
            k.rgba8[i] = (uint32_t)lroundf(VCT_CLEAR_R * 255.0f) | ((uint32_t)lroundf(VCT_CLEAR_G * 255.0f) << 8) |
                         ((uint32_t)lroundf(VCT_CLEAR_B * 255.0f) << 16) | (255u << 24);
        return;
    }
    const float4 N = k.nrm[i], A = k.alb[i], D = k.diff[i], S = k.spec[i];
    const float px = (P.x - k.g0x) * k.inv_h, py = (P.y - k.g0y) * k.inv_h, pz = (P.z - k.g0z) * k.inv_h;
    const float qx = px + N.x, qy = py + N.y, qz = pz + N.z;
    float dr = 0.0f, dg = 0.0f, db = 0.0f;
    for (uint32_t j = 0; j < k.n_lights; ++j) {
        const DLight& L = set.l[j];
        float lx, ly, lz, f, ndl, t_lim;
        if (!light_terms(L, k.h2, qx, qy, qz, N.x, N.y, N.z, lx, ly, lz, f, ndl, t_lim)) continue;
        float vis;
        if constexpr (VIS) vis = k.vis[(size_t)j * npx + i];
        else   // shadow-walk receiver rule (vct_spec.h): the float test before the walk's conversion
            vis = walk_starts(k.n, qx, qy, qz) ? dda_lim(k.bits, k.n, qx, qy, qz, lx, ly, lz, t_lim) : 1.0f;
        dr = dr + (((A.x * L.cr) * ndl) * f) * vis;
        dg = dg + (((A.y * L.cg) * ndl) * f) * vis;
        db = db + (((A.z * L.cb) * ndl) * f) * vis;
    }
    float fr = (dr + A.x * D.x) + S.x, fg = (dg + A.y * D.y) + S.y, fb = (db + A.z * D.z) + S.z;
    if constexpr (EM) {
        // Em = E of the voxel holding P itself (no normal offset); +0 outside the grid (a NaN
        // fails the compares) and at a voxel that does not emit
        float er = 0.0f, eg = 0.0f, eb = 0.0f;
        const float fn = (float)k.n;
        if (px >= 0.0f && px < fn && py >= 0.0f && py < fn && pz >= 0.0f && pz < fn) {
            const uint32_t v = (uint32_t)(int)floorf(px) +
                               (uint32_t)k.n * ((uint32_t)(int)floorf(py) + (uint32_t)k.n * (uint32_t)(int)floorf(pz));
            const unsigned long long word = k.em_bits[v >> 6];
            if ((word >> (v & 63u)) & 1ull) {
                const float4 e = k.em_E[bit_rank(k.em_prefix, v >> 6, word, v & 63u)];
                er = e.x; eg = e.y; eb = e.z;
            }
        }
        fr = fr + k.scale * er;
        fg = fg + k.scale * eg;
        fb = fb + k.scale * eb;
    }
    if (k.lin) k.lin[i] = make_float4(fr, fg, fb, 1.0f);
    if (k.rgba8) k.rgba8[i] = to8(fr) | (to8(fg) << 8) | (to8(fb) << 16) | (255u << 24);
}

// ---- host side --------------------------------------------------------------------------
// tool / test settings (vct_debug_lights), process-wide
std::atomic<int> g_form{-1};          // -1 the shipped form, 0 one light per pass, 1 batched pairs
std::atomic<uint32_t> g_pair_cap{0};  // entries of the pair list (0: default_pair_cap)
std::atomic<int> g_count{0};          // kl_walk counts the cells it tests
std::atomic<int> g_route{1};          // [directional] goes to launch_inject
constexpr int kShippedForm = 1;

// scratch slot 5: 256 bytes of counters, then the masks; slot 6: the pair list
constexpr int kSlotMask = 5, kSlotPairs = 6;
// counters: [0] pairs of the current batch, [1] pairs of the call, [2..3] cells (u64)

// Entries of the pair list.  A batch of nb lights makes at most nb pairs per occupied voxel,
// and the host does not know how many voxels are occupied (it never reads the count back);
// half an entry per voxel of the grid holds every pair of the scenes measured (surfaces:
// occupied voxels are a few percent of the grid), and kl_pairs walks what does not fit.
uint32_t default_pair_cap(size_t nv, uint32_t nb) {
    const size_t all = nv * nb;
    const size_t want = std::max<size_t>(nv / 2, (size_t)1 << 16);
    return (uint32_t)std::min<size_t>(std::min(all, want), 0xffffffffu);
}

hipError_t launch_lights(vct_ctx* c, const DLight* lights, uint32_t n_lights) {
    Grid& g = c->grid;
    const size_t nv = (size_t)g.n * g.n * g.n;
    const int lgn = __builtin_ctz(g.n);
    int cs = 0;
    while ((g.n >> cs) > 64) ++cs;
    const uint32_t cn = g.n >> cs;
    int form = g_form.load();
    if (form < 0) form = kShippedForm;
    // lights per batch: a mask bit each, and (index << lb | light) must fit 32 bits
    uint32_t nbmax = form == 0 ? 1u : (uint32_t)kBatch;
    while (nbmax > 1 && 3 * lgn + (32 - __builtin_clz(nbmax - 1)) > 32) nbmax >>= 1;
    const uint32_t lb = nbmax > 1 ? 32 - __builtin_clz(nbmax - 1) : 0;
    uint32_t cap = g_pair_cap.load();
    if (!cap) cap = default_pair_cap(nv, std::min(nbmax, std::max(n_lights, 1u)));
    hipStream_t s = c->stream;
    hipError_t e;
    const bool fresh = c->scratch[kSlotMask].bytes < 256 + nv * 4;
    void* sp = nullptr;
    if ((e = scratch_get(c, kSlotMask, 256 + nv * 4, &sp)) != hipSuccess) return e;
    uint32_t* counters = (uint32_t*)sp;
    uint32_t* mask = (uint32_t*)((char*)sp + 256);
    // the masks are zero between calls (kl_sum clears what kl_walk set): a new buffer once
    if (fresh && (e = hipMemsetAsync(mask, 0, nv * 4, s)) != hipSuccess) return e;
    void* pp = nullptr;
    if ((e = scratch_get(c, kSlotPairs, (size_t)cap * 4, &pp)) != hipSuccess) return e;
    uint32_t* pairs = (uint32_t*)pp;
    if ((e = hipMemsetAsync(counters, 0, 16, s)) != hipSuccess) return e;
    // level 0 is zero outside the occupied voxels unless a dense upload replaced it since
    if (g.l0_dense) {
        if ((e = hipMemsetAsync(g.pyr, 0, nv * sizeof(float4), s)) != hipSuccess) return e;
        g.l0_dense = false;
    }
    if (!g.k2_coarse_ok) {
        hipLaunchKernelGGL(kl_coarse, dim3((64 * cn * cn + 255) / 256), dim3(256), 0, s, g.occ_bits, (int)g.n, cs,
                           g.k2_coarse);
        g.k2_coarse_ok = true;
    }
    const float h2 = grid_h2(g);
    const uint32_t lane_blocks = (uint32_t)std::min<size_t>((nv / 16 + 255) / 256 + 1, 2048);
    const bool count = g_count.load() != 0;
    unsigned long long* cells = (unsigned long long*)(counters + 2);
    LightBatch batch;
    uint32_t done = 0;
    do {
        const uint32_t nb = std::min(nbmax, n_lights - done);
        std::memset(&batch, 0, sizeof batch);
        if (nb) std::memcpy(batch.l, lights + done, nb * sizeof(DLight));
        if (nb) {
            if (done && (e = hipMemsetAsync(counters, 0, 4, s)) != hipSuccess) return e;
            hipLaunchKernelGGL(kl_pairs, dim3(lane_blocks, nb), dim3(256), 0, s, g.occ_list, g.occ_count, g.normal,
                               g.occ_bits, lgn, batch, h2, lb, pairs, counters, cap, mask);
            if (count)
                hipLaunchKernelGGL((kl_walk<16, 256, true>), dim3(2048), dim3(256), 0, s, pairs, counters, cap, lb,
                                   g.occ_list, g.k2_coarse, cs, g.normal, g.occ_bits, lgn, batch, h2, mask, cells);
            else
                hipLaunchKernelGGL((kl_walk<16, 256, false>), dim3(2048), dim3(256), 0, s, pairs, counters, cap, lb,
                                   g.occ_list, g.k2_coarse, cs, g.normal, g.occ_bits, lgn, batch, h2, mask, cells);
        }
        hipLaunchKernelGGL(kl_sum, dim3(lane_blocks), dim3(256), 0, s, g.occ_list, g.occ_count, g.albedo_occ, g.normal,
                           lgn, batch, nb, h2, done == 0 ? 1 : 0, mask, counters, g.pyr);
        done += nb;
    } while (done < n_lights);
    return hipGetLastError();
}

}  // namespace

vct_status composite_light_list(vct_ctx* c, const char* what, const float* pos4, const float* nrm4, const float* alb4,
                                const float* diffuse4, const float* spec4, uint32_t w, uint32_t h,
                                const vct_light* lights, uint32_t n_lights, const CompositeForm& form,
                                float* out_linear4, uint32_t* out_rgba8) {
    if (!c || !pos4 || !nrm4 || !alb4 || !diffuse4 || !spec4 || w == 0 || h == 0) return VCT_EINVAL;
    if (!out_linear4 && !out_rgba8) return lfail(c, VCT_EINVAL, "composite: no output");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "composite: frame too large");
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "composite before voxelize");
    for (const void* p : {(const void*)pos4, (const void*)nrm4, (const void*)alb4, (const void*)diffuse4,
                          (const void*)spec4, (const void*)out_linear4})
        if (((uintptr_t)p & 15u) != 0) return lfail(c, VCT_EINVAL, "composite: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)out_rgba8 & 3u) != 0) return lfail(c, VCT_EINVAL, "composite: rgba8 buffer must be 4-byte aligned");
    if (form.own_error) return lfail(c, VCT_EINVAL, std::string(what) + ": " + form.own_error);
    LightSet set;
    std::memset(&set, 0, sizeof set);
    vct_status st = prepare_list(c, what, lights, n_lights, set.l);
    if (st != VCT_OK) return st;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    const Grid& g = c->grid;
    const Emission& em = c->em;
    CompK k;
    std::memset(&k, 0, sizeof k);
    k.pos = (const float4*)pos4; k.nrm = (const float4*)nrm4; k.alb = (const float4*)alb4;
    k.diff = (const float4*)diffuse4; k.spec = (const float4*)spec4;
    k.vis = form.vis;
    k.bits = g.occ_bits;
    k.em_bits = em.bits; k.em_prefix = em.prefix; k.em_E = em.E;
    k.n = (int)g.n; k.w = (int)w; k.h = (int)h;
    k.g0x = g.g0[0]; k.g0y = g.g0[1]; k.g0z = g.g0[2]; k.inv_h = g.inv_h; k.h2 = grid_h2(g);
    k.scale = form.scale;
    k.n_lights = n_lights;
    k.lin = (float4*)out_linear4; k.rgba8 = out_rgba8;
    const dim3 grid((w * h + 255) / 256), block(256);
    if (form.read_vis) {
        if (form.emit) hipLaunchKernelGGL((kl_composite<true, true>), grid, block, 0, c->stream, k, set);
        else hipLaunchKernelGGL((kl_composite<true, false>), grid, block, 0, c->stream, k, set);
    } else {
        if (form.emit) hipLaunchKernelGGL((kl_composite<false, true>), grid, block, 0, c->stream, k, set);
        else hipLaunchKernelGGL((kl_composite<false, false>), grid, block, 0, c->stream, k, set);
    }
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, what);
    return VCT_OK;
}

}  // namespace vct

using namespace vct;

extern "C" vct_status vct_inject_lights(vct_ctx* c, const vct_light* lights, uint32_t n_lights) {
    if (!c) return VCT_EINVAL;
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "inject_lights before voxelize");
    DLight dl[VCT_MAX_LIGHTS];
    vct_status st = prepare_list(c, "inject_lights", lights, n_lights, dl);
    if (st != VCT_OK) return st;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    if (n_lights == 1 && dl[0].type == VCT_LIGHT_DIRECTIONAL && g_route.load())
        e = launch_inject(c, dl[0].ax, dl[0].ay, dl[0].az, dl[0].cr, dl[0].cg, dl[0].cb);   // K2 as it is
    else
        e = launch_lights(c, dl, n_lights);
    if (e != hipSuccess) return lhip(c, e, "inject_lights");
    c->grid.injected = true;
    c->grid.bounced = c->grid.emitted = c->grid.skied = false;
    c->grid.mipped = false;
    c->grid.l0_on_peers = false;
    return VCT_OK;
}

extern "C" vct_status vct_composite_lights_device(vct_ctx* c, const float* pos4, const float* nrm4, const float* alb4,
                                                  const float* diffuse4, const float* spec4, uint32_t w, uint32_t h,
                                                  const vct_light* lights, uint32_t n_lights, float* out_linear4,
                                                  uint32_t* out_rgba8) {
    return composite_light_list(c, "composite_lights", pos4, nrm4, alb4, diffuse4, spec4, w, h, lights, n_lights,
                                CompositeForm{}, out_linear4, out_rgba8);
}

// Tool / test hooks (not part of the public headers; tools/lights_bench.py, tests): the form
// vct_inject_lights runs (-1 the shipped one, 0 one light per pass, 1 batched pairs), the
// capacity of the pair list in entries (0: the default), cell counting in kl_walk, and
// whether a list of exactly one directional light is routed to vct_inject_directional's
// kernels.  Process-wide.
extern "C" void vct_debug_lights(int form, uint32_t pair_cap, int count, int route) {
    g_form.store(form < 0 ? -1 : (form ? 1 : 0));
    g_pair_cap.store(pair_cap);
    g_count.store(count);
    g_route.store(route);
}

// out[0] = pairs that needed a walk, out[1] = cells tested (with counting on; pairs walked by
// kl_pairs itself past the list's capacity are not counted) in the context's last
// vct_inject_lights through the light kernels.  Waits for the ctx stream.
extern "C" int vct_debug_lights_stats(vct_ctx* c, unsigned long long* out) {
    if (!c || !out || !c->scratch[kSlotMask].p) return -1;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    uint32_t w[4];
    if (hipMemcpy(w, c->scratch[kSlotMask].p, 16, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    out[0] = w[1];
    out[1] = (unsigned long long)w[2] | ((unsigned long long)w[3] << 32);
    return 0;
}
