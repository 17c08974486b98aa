// vct_voxel_sat.h — what the translation units that run K1's conservative voxelization
// pass share (vct_voxelize.hip: K1; vct_emission.hip: the emission grid; vct_dynamic.hip: the
// dynamic layer): the per-triangle candidate record and range, the exclusive scan of the
// candidate counts, the 32-bit block scan of the list and prefix kernels, the exact 13-axis
// SAT, the bucket table of the candidates kernel, the list of a bit mask's set bits and the
// resolve of one accumulator record.  Everything is internal to the
// including translation unit (vct_spec.h "K1 input rule" has the arithmetic).
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

constexpr int kCandPerThread = 8;
constexpr int kCandBucket = 512;                 // candidates per bucket of the triangle-lookup table

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

}  // namespace
}  // namespace vct
