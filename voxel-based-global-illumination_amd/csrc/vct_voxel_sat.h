// vct_voxel_sat.h — what the translation units that run K1's conservative voxelization
// pass share (vct_voxelize.hip: K1; vct_emission.hip: the emission grid; vct_dynamic.hip: the
// dynamic layer): the per-triangle candidate record, the pieces of the triangle setup (vertex
// load and q, the finiteness rule, the candidate range and count, the face normal and the 16.16
// values with their max|value|, the triangle the G-buffer passes read, the rejected record),
// the exclusive scan of the candidate counts, the walk over the flat candidate list (triangle
// search, decode, the exact 13-axis SAT), the bucket table of the candidates kernels, the
// 32-bit block scan of the list and prefix kernels, the list of a bit mask's set bits, the
// resolve of one accumulator record, and the host side of a pass (the layout of the triangle
// temporaries, the scan and bucket-table launches).  Each unit keeps its own three kernels and
// what is its own in them.  Everything is internal to the including translation unit
// (vct_spec.h "K1 input rule" has the arithmetic; the order of the float operations here is
// part of it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vct_internal.h"
#include "vct_device.h"

namespace vct {
namespace {

struct TriGeom {      // 64 B
    float q[9];       // voxel-unit vertex positions
    int lo[3];        // first candidate voxel per axis
    uint32_t ext[3];  // candidate extent per axis (0 = no candidates)
    uint32_t pad;
};

// K1's per-triangle records beside TriGeom (vct_voxelize.hip; vct_cutout.hip fills the pads)
struct TriFix {       // 64 B
    long long fix[6]; // albedo rgb, face normal xyz in 16.16 fixed point
    long long tex;    // diffuse map of the triangle's material (-1: albedo = Kd, fix[0..2])
    long long pad;    // K1 with cutouts: the mask word, 4 * mask map + channel (-1: opaque); else 0
};
struct TriUV {        // 48 B, textured (K1 with cutouts: and masked) triangles only
    float uv[6];      // TexCoords of the three vertices
    float kd[3];      // material Kd (albedo = Kd x T(uv) per hit)
    uint32_t pad[3];  // K1 with cutouts: [0] = the cutoff's bits; else 0
};

__device__ __forceinline__ float fmin3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float fmax3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// vct_spec.h "K1 input rule": both ends clamped to [-1, n + 1] before the conversion
__device__ __forceinline__ void cand_range(float mn, float mx, int n, int& lo, int& hi) {
    const float top = (float)n + 1.0f;
    int l = (int)ceilf(fminf(fmaxf(mn, -1.0f), top)) - 1;
    int h = (int)floorf(fmaxf(fminf(mx, top), -1.0f));
    lo = l < 0 ? 0 : l;
    hi = h > n - 1 ? n - 1 : h;
}

// ---- the triangle setup ---------------------------------------------------------------------
// Triangle t's vertex indices, range-checked (false: one is out of range, nothing is loaded),
// its vertices p (world units) and q = (p - g0) * inv_h (voxel units).  All nine loads are
// issued before the caller's first test of a value, so that they are in flight together.
__device__ __forceinline__ bool load_tri(const char* __restrict__ verts, uint32_t stride, uint32_t n_verts,
                                         const uint32_t* __restrict__ idx, uint32_t t, float g0x, float g0y, float g0z,
                                         float inv_h, uint32_t vi[3], float p[3][3], float q[3][3]) {
    vi[0] = idx[3 * t]; vi[1] = idx[3 * t + 1]; vi[2] = idx[3 * t + 2];
    if (vi[0] >= n_verts || vi[1] >= n_verts || vi[2] >= n_verts) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* src = (const float*)(verts + (size_t)vi[k] * stride);
        p[k][0] = src[0]; p[k][1] = src[1]; p[k][2] = src[2];
        q[k][0] = (p[k][0] - g0x) * inv_h;
        q[k][1] = (p[k][1] - g0y) * inv_h;
        q[k][2] = (p[k][2] - g0z) * inv_h;
    }
    return true;
}

// K1 input rule: a triangle with a non-finite q is skipped (NaN fails the compare)
// (`&`, not `&&`: short-circuit evaluation would make each load wait for the one before it)
__device__ __forceinline__ bool tri_finite(const float q[3][3]) {
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        finite &= ((int)(fabsf(q[k][0]) < __builtin_inff()) & (int)(fabsf(q[k][1]) < __builtin_inff()) &
                   (int)(fabsf(q[k][2]) < __builtin_inff())) != 0;
    return finite;
}

// q and the candidate range into the record; returns the candidate count
__device__ __forceinline__ unsigned long long tri_range(const float q[3][3], int n, TriGeom& g) {
    unsigned long long cnt = 1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int lo, hi;
        cand_range(fmin3(q[0][a], q[1][a], q[2][a]), fmax3(q[0][a], q[1][a], q[2][a]), n, lo, hi);
        g.lo[a] = lo;
        g.ext[a] = hi >= lo ? (uint32_t)(hi - lo + 1) : 0u;
        cnt *= g.ext[a];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { g.q[3 * k] = q[k][0]; g.q[3 * k + 1] = q[k][1]; g.q[3 * k + 2] = q[k][2]; }
    g.pad = 0;
    return cnt;
}

// the edge vectors e1, e2 (world units), the unit face normal (0 for a degenerate triangle) and
// the six 16.16 values of a hit: albedo rgb, normal xyz
__device__ __forceinline__ void face_fix(const float p[3][3], const float4 alb, long long fix[6], float e1[3],
                                         float e2[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { e1[a] = p[1][a] - p[0][a]; e2[a] = p[2][a] - p[0][a]; }
    float fn[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                   e1[0] * e2[1] - e1[1] * e2[0]};
    float len = sqrtf(dot3(fn[0], fn[1], fn[2], fn[0], fn[1], fn[2]));
    if (len > 0.0f) { fn[0] = fn[0] / len; fn[1] = fn[1] / len; fn[2] = fn[2] / len; }
    else { fn[0] = 0.0f; fn[1] = 0.0f; fn[2] = 0.0f; }
    fix[0] = (long long)roundf(alb.x * VCT_FIXED_ONE);
    fix[1] = (long long)roundf(alb.y * VCT_FIXED_ONE);
    fix[2] = (long long)roundf(alb.z * VCT_FIXED_ONE);
    fix[3] = (long long)roundf(fn[0] * VCT_FIXED_ONE);
    fix[4] = (long long)roundf(fn[1] * VCT_FIXED_ONE);
    fix[5] = (long long)roundf(fn[2] * VCT_FIXED_ONE);
}

// *maxabs = max(*maxabs, the largest |fixed-point value| a hit of this triangle adds), clamped
// at 2^31 (a textured albedo Kd x T with T <= 1 rounds to at most Kd's).  The plain load first:
// nearly every triangle is below the maximum already and issues no atomic
__device__ __forceinline__ void fix_maxabs(const long long fix[6], uint32_t* __restrict__ maxabs) {
    unsigned long long mx = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const unsigned long long a = (unsigned long long)(fix[i] < 0 ? -fix[i] : fix[i]);
        mx = a > mx ? a : mx;
    }
    const uint32_t m32 = mx >= (1ull << 31) ? (1u << 31) : (uint32_t)mx;
    if (m32 > __hip_atomic_load(maxabs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(maxabs, m32);
}

// the triangle the G-buffer passes read (world units): v0, e1, e2, (kd rgb, diffuse map; -1 none).
// A skipped triangle is stored with v0 = e1 = e2 = 0, which no ray hits
__device__ __forceinline__ void store_mesh_tri(float4* __restrict__ mesh_tri, uint32_t t, const float v0[3],
                                               const float e1[3], const float e2[3], const float4 alb, int tex) {
    mesh_tri[4 * t + 0] = make_float4(v0[0], v0[1], v0[2], 0.0f);
    mesh_tri[4 * t + 1] = make_float4(e1[0], e1[1], e1[2], 0.0f);
    mesh_tri[4 * t + 2] = make_float4(e2[0], e2[1], e2[2], 0.0f);
    mesh_tri[4 * t + 3] = make_float4(alb.x, alb.y, alb.z, __int_as_float(tex));
}

// A triangle without candidates (an index out of range, a broken material rule, a non-finite
// q, nothing to add): count 0 and an all-zero record.  No candidates kernel visits such a
// triangle, so neither its record nor its fixed-point values are ever read
__device__ __forceinline__ void reject_tri(TriGeom* __restrict__ geom, unsigned long long* __restrict__ counts,
                                           uint32_t t) {
    TriGeom g;
#pragma unroll
    for (int i = 0; i < 9; ++i) g.q[i] = 0.0f;
    g.lo[0] = g.lo[1] = g.lo[2] = 0;
    g.ext[0] = g.ext[1] = g.ext[2] = 0;
    g.pad = 0;
    geom[t] = g;
    counts[t] = 0;
}

// ---- exclusive scan of per-triangle candidate counts (u64) ----------------
constexpr int kScanBlock = 256, kScanItems = 4, kScanTile = kScanBlock * kScanItems;

__device__ __forceinline__ unsigned long long block_excl_scan(unsigned long long v,
                                                             unsigned long long* sh,
                                                             unsigned long long& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned long long x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        unsigned long long y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) sh[wid] = x;
    __syncthreads();
    unsigned long long base = 0;
    for (int w = 0; w < wid; ++w) base += sh[w];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return base + x - v;
}

__global__ void __launch_bounds__(kScanBlock) k_scan_tiles(const unsigned long long* __restrict__ in,
                                                           unsigned long long* __restrict__ out,
                                                           unsigned long long* __restrict__ tile_sums,
                                                           uint32_t count) {
    __shared__ unsigned long long sh[4];
    const size_t base = (size_t)blockIdx.x * kScanTile + (size_t)threadIdx.x * kScanItems;
    unsigned long long v[kScanItems], s = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
        v[i] = base + i < count ? in[base + i] : 0ull;
        s += v[i];
    }
    unsigned long long total;
    unsigned long long ex = block_excl_scan(s, sh, total);
#pragma unroll
    for (int i = 0; i < kScanItems; ++i) {
        if (base + i < count) out[base + i] = ex;
        ex += v[i];
    }
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// single-block carry scan over the tile sums (n_tiles small: n_tri / 1024)
__global__ void __launch_bounds__(kScanBlock) k_scan_carry(unsigned long long* __restrict__ tile_sums,
                                                           uint32_t n_tiles,
                                                           unsigned long long* __restrict__ total_out) {
    __shared__ unsigned long long sh[4];
    unsigned long long carry = 0;
    for (uint32_t b = 0; b < n_tiles; b += kScanBlock) {
        uint32_t i = b + threadIdx.x;
        unsigned long long v = i < n_tiles ? tile_sums[i] : 0ull, tot;
        unsigned long long ex = block_excl_scan(v, sh, tot);
        if (i < n_tiles) tile_sums[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ void __launch_bounds__(kScanBlock) k_scan_add(unsigned long long* __restrict__ out,
                                                         const unsigned long long* __restrict__ tile_sums,
                                                         uint32_t count) {
    const size_t base = (size_t)blockIdx.x * kScanTile;
    const unsigned long long add = tile_sums[blockIdx.x];
    for (int i = threadIdx.x; i < kScanTile; i += kScanBlock)
        if (base + i < count) out[base + i] += add;
}

// exclusive prefix sum of one value per thread over a 256-thread block, and the
// block total (4 waves: shuffles within the wave, wave totals through LDS)
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t& total) {
    __shared__ uint32_t wt[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += t;
    }
    if (lane == 63) wt[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += wt[w];
    total = wt[0] + wt[1] + wt[2] + wt[3];
    __syncthreads();
    return before + incl - v;
}

// ---- exact 13-axis triangle/voxel SAT (same rule as oracle/vct_oracle.c) --
__device__ __forceinline__ bool tri_box_overlap(const float* __restrict__ q, float cx, float cy, float cz) {
    float a0x = q[0] - cx, a0y = q[1] - cy, a0z = q[2] - cz;
    float a1x = q[3] - cx, a1y = q[4] - cy, a1z = q[5] - cz;
    float a2x = q[6] - cx, a2y = q[7] - cy, a2z = q[8] - cz;
    if (fmin3(a0x, a1x, a2x) > 0.5f || fmax3(a0x, a1x, a2x) < -0.5f) return false;
    if (fmin3(a0y, a1y, a2y) > 0.5f || fmax3(a0y, a1y, a2y) < -0.5f) return false;
    if (fmin3(a0z, a1z, a2z) > 0.5f || fmax3(a0z, a1z, a2z) < -0.5f) return false;
    float e[3][3] = {{a1x - a0x, a1y - a0y, a1z - a0z},
                     {a2x - a1x, a2y - a1y, a2z - a1z},
                     {a0x - a2x, a0y - a2y, a0z - a2z}};
    {
        float nx = e[0][1] * e[1][2] - e[0][2] * e[1][1];
        float ny = e[0][2] * e[1][0] - e[0][0] * e[1][2];
        float nz = e[0][0] * e[1][1] - e[0][1] * e[1][0];
        float vminx, vmaxx, vminy, vmaxy, vminz, vmaxz;
        if (nx > 0.0f) { vminx = -0.5f - a0x; vmaxx = 0.5f - a0x; } else { vminx = 0.5f - a0x; vmaxx = -0.5f - a0x; }
        if (ny > 0.0f) { vminy = -0.5f - a0y; vmaxy = 0.5f - a0y; } else { vminy = 0.5f - a0y; vmaxy = -0.5f - a0y; }
        if (nz > 0.0f) { vminz = -0.5f - a0z; vmaxz = 0.5f - a0z; } else { vminz = 0.5f - a0z; vmaxz = -0.5f - a0z; }
        if (dot3(nx, ny, nz, vminx, vminy, vminz) > 0.0f) return false;
        if (!(dot3(nx, ny, nz, vmaxx, vmaxy, vmaxz) >= 0.0f)) return false;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float ex = e[i][0], ey = e[i][1], ez = e[i][2];
        const float ax[3][3] = {{0.0f, -ez, ey}, {ez, 0.0f, -ex}, {-ey, ex, 0.0f}};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float ux = ax[j][0], uy = ax[j][1], uz = ax[j][2];
            float p0 = dot3(ux, uy, uz, a0x, a0y, a0z);
            float p1 = dot3(ux, uy, uz, a1x, a1y, a1z);
            float p2 = dot3(ux, uy, uz, a2x, a2y, a2z);
            float rad = 0.5f * ((fabsf(ux) + fabsf(uy)) + fabsf(uz));
            if (fmin3(p0, p1, p2) > rad || fmax3(p0, p1, p2) < -rad) return false;
        }
    }
    return true;
}

// ---- the walk over the flat candidate list ----------------------------------------------------
constexpr int kCandPerThread = 8;
constexpr int kCandBucket = 512;                 // candidates per bucket of the triangle-lookup table

// The triangle holding candidate c0: the last t of [lo, hi) with offs[t] <= c0 (offs[lo] <= c0).
// Zero-count triangles share their successor's offset, so the search lands past them
__device__ __forceinline__ uint32_t find_tri(const unsigned long long* __restrict__ offs, uint32_t lo, uint32_t hi,
                                             unsigned long long c0) {
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offs[mid] <= c0) lo = mid; else hi = mid;
    }
    return lo;
}

// The same, searched between the triangles of c0's bucket start and of the next bucket's start
// (starts: k1_bucket_starts' table): a few steps instead of log2(n_tri) dependent loads.
// starts[bk] holds candidate bk * kCandBucket <= c0, and c0's triangle is at most
// starts[bk + 1], so the window has it
__device__ __forceinline__ uint32_t find_tri_bucketed(const unsigned long long* __restrict__ offs,
                                                      const uint32_t* __restrict__ starts, uint32_t n_tri,
                                                      unsigned long long total, unsigned long long c0) {
    const unsigned long long bk = c0 / kCandBucket, nbk = (total + kCandBucket - 1) / kCandBucket;
    return find_tri(offs, starts[bk], bk + 1 < nbk ? starts[bk + 1] + 1 : n_tri, c0);
}

// CPT consecutive candidates from c0, which triangle t holds: each one's voxel (x fastest in
// the triangle's candidate box) through the SAT; hit(t, vx, vy, vz, q) for those that pass.
// Every index is bounded: t < n_tri by the search over offs[0 .. n_tri), the voxel by
// cand_range's clamp to [0, n - 1]
template <int CPT, typename Hit>
__device__ __forceinline__ void for_each_hit(const TriGeom* __restrict__ geom,
                                             const unsigned long long* __restrict__ offs, uint32_t n_tri,
                                             unsigned long long total, unsigned long long c0, uint32_t t, Hit&& hit) {
    unsigned long long next = t + 1 < n_tri ? offs[t + 1] : total;
    for (int k = 0; k < CPT; ++k) {
        const unsigned long long c = c0 + k;
        if (c >= total) break;
        while (c >= next) { ++t; next = t + 1 < n_tri ? offs[t + 1] : total; }
        const TriGeom& g = geom[t];
        const unsigned long long local = c - offs[t];
        const uint32_t ex = g.ext[0], ey = g.ext[1];
        const uint32_t x = (uint32_t)(local % ex);
        const unsigned long long r = local / ex;
        const uint32_t y = (uint32_t)(r % ey);
        const uint32_t z = (uint32_t)(r / ey);
        const int vx = g.lo[0] + (int)x, vy = g.lo[1] + (int)y, vz = g.lo[2] + (int)z;
        float q[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) q[i] = g.q[i];
        if (tri_box_overlap(q, (float)vx + 0.5f, (float)vy + 0.5f, (float)vz + 0.5f)) hit(t, vx, vy, vz, q);
    }
}

// ---- the occupied list from a bit mask ------------------------------------------------------
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The set bits of a 256-thread block's words (thread's word `mine` is word w of the mask, 0
// past its end) appended to `list` in bitmask order: per word, lane j owns bit j (ballot +
// mbcnt give coalesced slots), one atomic per block.  Every thread of the block calls it.
__device__ __forceinline__ void list_block_words(unsigned long long mine, size_t w, uint32_t* __restrict__ list,
                                                 uint32_t* __restrict__ count) {
    __shared__ uint32_t s_base;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t total;
    const uint32_t excl = block_excl_scan((uint32_t)__popcll(mine), total);
    if (total == 0) return;                                  // block-uniform
    if (threadIdx.x == 0) s_base = atomicAdd(count, total);
    __syncthreads();
    const uint32_t base = s_base;
    const size_t w0 = w - lane;                              // the wave's first word
    for (int i = 0; i < 64; ++i) {
        const unsigned long long m =
            ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), i) << 32) |
            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, i);
        if (m == 0ull) continue;
        const uint32_t start = base + (uint32_t)__builtin_amdgcn_readlane((int)excl, i);
        if ((m >> lane) & 1ull) list[start + lanes_below(m)] = (uint32_t)((w0 + i) * 64 + lane);
    }
}

// ---- K1's accumulator record -> the resolved voxel -------------------------------------------
// a packed word's two sums (|sum| < 2^31 each)
__host__ __device__ __forceinline__ void unpack_sums(long long w, long long& lo, long long& hi) {
    lo = (long long)(int32_t)(uint32_t)(unsigned long long)w;
    hi = (long long)(((unsigned long long)w - (unsigned long long)lo)) >> 32;
}

// PACKED: a voxel whose count x maxabs could reach 2^31 ORs kK1ErrRedo into *overflow and is
// left as it was (its packed sums cannot be trusted)
template <bool PACKED>
__device__ __forceinline__ void resolve_voxel(const long long* __restrict__ accum, size_t v,
                                              float4* __restrict__ albedo_occ, float4* __restrict__ normal,
                                              uint32_t maxabs, int* __restrict__ overflow) {
    long long s[7];
    {
        const longlong2* a = (const longlong2*)(accum + 8 * v);
        longlong2 p0 = a[0], p1 = a[1], p2 = a[2], p3 = a[3];
        if constexpr (PACKED) {
            s[6] = p1.y;
            if ((unsigned long long)s[6] * maxabs >= (1ull << 31)) {
                atomicOr(overflow, kK1ErrRedo);
                return;
            }
            unpack_sums(p0.x, s[0], s[1]);
            unpack_sums(p0.y, s[2], s[3]);
            unpack_sums(p1.x, s[4], s[5]);
        } else {
            s[0] = p0.x; s[1] = p0.y; s[2] = p1.x; s[3] = p1.y; s[4] = p2.x; s[5] = p2.y; s[6] = p3.x;
        }
    }
    const unsigned long long cnt = (unsigned long long)s[6];
    double den = (double)cnt * VCT_FIXED_ONE_D;
    float4 ao = make_float4((float)((double)s[0] / den), (float)((double)s[1] / den),
                            (float)((double)s[2] / den), 1.0f);
    double sx = (double)s[3], sy = (double)s[4], sz = (double)s[5];
    double len = sqrt((sx * sx + sy * sy) + sz * sz);
    float4 nm = len > 0.0 ? make_float4((float)(sx / len), (float)(sy / len), (float)(sz / len), 0.0f)
                          : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    albedo_occ[v] = ao;
    normal[v] = nm;
}

// bucket b -> the triangle holding candidate b * kCandBucket (triangles whose
// candidate range crosses a bucket start write it; a giant triangle writes many)
__global__ void __launch_bounds__(256) k1_bucket_starts(const unsigned long long* __restrict__ offs, uint32_t n_tri,
                                                        const unsigned long long* __restrict__ total_p,
                                                        uint32_t* __restrict__ starts) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tri) return;
    const unsigned long long lo = offs[t], hi = t + 1 < n_tri ? offs[t + 1] : *total_p;
    if (hi <= lo) return;                        // no candidates
    for (unsigned long long b = (lo + kCandBucket - 1) / kCandBucket; b * kCandBucket < hi; ++b) starts[b] = t;
}

// ---- host side of a pass ------------------------------------------------------------------------
// The triangle temporaries of a pass (vct_ctx::scratch slot 1):
//   geom | fix | counts | offsets | tile sums | head (64 bytes) | tail (256-byte aligned)
struct TriTemps {
    TriGeom* geom;
    void* fix;                                    // n_tri records of fix_bytes
    unsigned long long *counts, *offs, *tiles;
    void* head;                                   // the pass's words on the device: total, max|value|, error ...
    void* tail;                                   // tail_bytes (K1: the textured triangles' UVs)
};

hipError_t tri_temps(vct_ctx* c, uint32_t n_tri, size_t fix_bytes, size_t tail_bytes, TriTemps& t) {
    const uint32_t n_tiles = (n_tri + kScanTile - 1) / kScanTile;
    const size_t off_fix = sizeof(TriGeom) * (size_t)n_tri;
    const size_t off_cnt = off_fix + fix_bytes * (size_t)n_tri;
    const size_t off_offs = off_cnt + 8 * (size_t)n_tri;
    const size_t off_tiles = off_offs + 8 * (size_t)n_tri;
    const size_t off_head = off_tiles + 8 * (size_t)(n_tiles + 1);
    const size_t off_tail = (off_head + 64 + 255) & ~(size_t)255;
    void* sp;
    hipError_t e = scratch_get(c, 1, off_tail + tail_bytes, &sp);
    if (e != hipSuccess) return e;
    char* base = (char*)sp;
    t.geom = (TriGeom*)base;
    t.fix = base + off_fix;
    t.counts = (unsigned long long*)(base + off_cnt);
    t.offs = (unsigned long long*)(base + off_offs);
    t.tiles = (unsigned long long*)(base + off_tiles);
    t.head = base + off_head;
    t.tail = base + off_tail;
    return hipSuccess;
}

// offs = the exclusive scan of n_tri counts, *total_out their sum (all device); tiles: n_tri /
// kScanTile + 1 words
void launch_count_scan(hipStream_t s, const unsigned long long* counts, unsigned long long* offs,
                       unsigned long long* tiles, uint32_t n_tri, unsigned long long* total_out) {
    const uint32_t n_tiles = (n_tri + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(k_scan_tiles, dim3(n_tiles), dim3(kScanBlock), 0, s, counts, offs, tiles, n_tri);
    hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(kScanBlock), 0, s, tiles, n_tiles, total_out);
    hipLaunchKernelGGL(k_scan_add, dim3(n_tiles), dim3(kScanBlock), 0, s, offs, (const unsigned long long*)tiles, n_tri);
}

// The launch shape of a candidates kernel that takes kCandPerThread per lane for h_total > 0
// candidates (the host's copy of *total), and the bucket table (vct_ctx::scratch slot 7), queued.
// hipErrorInvalidValue, with nothing done: more blocks than a launch takes
hipError_t launch_bucket_starts(vct_ctx* c, const unsigned long long* offs, uint32_t n_tri,
                                const unsigned long long* total, unsigned long long h_total, uint32_t* blocks,
                                uint32_t** starts) {
    const unsigned long long threads = (h_total + kCandPerThread - 1) / kCandPerThread;
    const unsigned long long b = (threads + 255) / 256;
    if (b > 0x7fffffffull) return hipErrorInvalidValue;
    const unsigned long long nbk = (h_total + kCandBucket - 1) / kCandBucket;
    void* bp;
    hipError_t e = scratch_get(c, 7, (size_t)nbk * 4, &bp);
    if (e != hipSuccess) return e;
    *blocks = (uint32_t)b;
    *starts = (uint32_t*)bp;
    hipLaunchKernelGGL(k1_bucket_starts, dim3((n_tri + 255) / 256), dim3(256), 0, c->stream, offs, n_tri, total,
                       *starts);
    return hipSuccess;
}

}  // namespace
}  // namespace vct
