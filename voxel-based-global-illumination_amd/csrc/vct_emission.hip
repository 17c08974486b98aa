// vct_emission.hip — emissive surfaces (include/vct_emission.h; the arithmetic is
// include/vct_spec.h "emissive surfaces"): the emission grid E of a voxelization, its add
// into level 0, and the composite that shows it.
//
// The build is a K1-shaped pass over the emitter triangles (vct_voxel_sat.h: the same
// candidate range, scan, bucket table and SAT as K1):
//   k_em_setup       one lane per triangle: q, candidate range and the three 16.16 values of
//                    its material's Ke; a triangle with Ke = 0 or a non-finite q gets no
//                    candidates, so the cost follows the emitters, not the mesh.  The Ke rule
//                    and the index ranges are checked here (the error word).
//   k_bits_prefix_*  exclusive scan of popc over a bit mask's words: applied to K1's occupancy
//                    bits it gives every occupied voxel a dense rank (and their number, read
//                    back with the candidate total in the call's one wait), applied to the
//                    emissive bits it gives the composite its O(1) lookup.
//   k_em_candidates  one lane per 8 (triangle, voxel) candidates: the SAT, then for a hit in
//                    an occupied voxel three 64-bit integer atomics into the sums of that
//                    voxel's rank.  A hit in an empty voxel (count = 0) is dropped.  Integer
//                    sums do not depend on the arrival order: the grid is bit-exact.
//   k_em_mark        one lane per occupied voxel: a nonzero sum sets the voxel's emissive bit.
//   k_em_resolve     one lane per occupied voxel: an emissive one writes its index and
//                    E = S / (count * 2^16) (float64 divide, as k1_resolve) at its emissive
//                    rank, with count read from K1's accumulator record.
//   k_em_add         one lane per emissive voxel: level 0 += scale * E, at K2's texel.
//   k_em_composite   kl_composite / ks_composite (walked or read V) plus scale * E of the
//                    pixel's voxel.
// Memory: the sums and the compact arrays are sized by the occupied voxels (44 bytes each);
// only the bit and prefix words are sized by the grid (3 n^3 / 16 bytes).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include "vct_internal.h"
#include "vct_voxel_sat.h"
#include "vct_light_terms.h"

namespace vct {
namespace {

constexpr int kEmErrIndex = 1, kEmErrKe = 2;
constexpr int kSlotTri = 1, kSlotBuckets = 7, kSlotRank = 11;   // vct_ctx::scratch (1 and 7 as K1 uses them)

struct EmFix {        // 32 B
    long long fix[3]; // Ke rgb in 16.16 fixed point
    long long pad;
};

struct EmHead {       // read back once per build
    unsigned long long total;   // candidates
    uint32_t n_occ;             // occupied voxels (set bits of K1's occupancy)
    int err;
};

// the Ke rule (vct_spec.h "emissive surfaces"): finite, sign bit clear, < VCT_KD_LIMIT
__host__ __device__ __forceinline__ bool ke_legal(float k) {
    return k >= 0.0f && k < VCT_KD_LIMIT && (__builtin_bit_cast(uint32_t, k) >> 31) == 0u;
}

__global__ void __launch_bounds__(256) k_em_setup(const char* __restrict__ verts, uint32_t stride, uint32_t n_verts,
                                                  const uint32_t* __restrict__ idx, uint32_t n_tri,
                                                  const uint32_t* __restrict__ mat, const float4* __restrict__ ke,
                                                  uint32_t n_mat, int n, float g0x, float g0y, float g0z, float inv_h,
                                                  TriGeom* __restrict__ geom, EmFix* __restrict__ fixo,
                                                  unsigned long long* __restrict__ counts, int* __restrict__ err) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tri) return;
    const uint32_t vi[3] = {idx[3 * t], idx[3 * t + 1], idx[3 * t + 2]};
    const uint32_t m = mat ? mat[t] : 0u;
    TriGeom g;
    g.lo[0] = g.lo[1] = g.lo[2] = 0;
    g.ext[0] = g.ext[1] = g.ext[2] = 0;
    g.pad = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) g.q[i] = 0.0f;
    if (vi[0] >= n_verts || vi[1] >= n_verts || vi[2] >= n_verts || m >= n_mat) {
        atomicOr(err, kEmErrIndex);
        geom[t] = g;
        counts[t] = 0;
        return;
    }
    const float4 k4 = ke[m];
    float q[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* src = (const float*)(verts + (size_t)vi[k] * stride);
        q[k][0] = (src[0] - g0x) * inv_h;
        q[k][1] = (src[1] - g0y) * inv_h;
        q[k][2] = (src[2] - g0z) * inv_h;
    }
    if (!(ke_legal(k4.x) && ke_legal(k4.y) && ke_legal(k4.z))) {
        atomicOr(err, kEmErrKe);
        geom[t] = g;
        counts[t] = 0;
        return;
    }
    EmFix f;
    f.fix[0] = (long long)roundf(k4.x * VCT_FIXED_ONE);
    f.fix[1] = (long long)roundf(k4.y * VCT_FIXED_ONE);
    f.fix[2] = (long long)roundf(k4.z * VCT_FIXED_ONE);
    f.pad = 0;
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        finite &= (fabsf(q[k][0]) < __builtin_inff()) & (fabsf(q[k][1]) < __builtin_inff()) &
                  (fabsf(q[k][2]) < __builtin_inff());
    // K1 input rule: a non-finite q is skipped; a triangle that emits nothing has no candidates
    if (!finite || (f.fix[0] | f.fix[1] | f.fix[2]) == 0) {
        geom[t] = g;
        counts[t] = 0;
        return;
    }
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
    geom[t] = g;
    fixo[t] = f;
    counts[t] = cnt;
}

// ---- exclusive scan of popc(word) over a bit mask (u32; n^3 <= 2^30 bits) --------------
constexpr int kPrefTile = 1024;   // words per block: 256 threads x 4

__global__ void __launch_bounds__(256) k_bits_prefix_tiles(const unsigned long long* __restrict__ bits, uint32_t nwords,
                                                           uint32_t* __restrict__ prefix,
                                                           uint32_t* __restrict__ tile_sums) {
    const uint32_t base = blockIdx.x * (uint32_t)kPrefTile + threadIdx.x * 4u;
    uint32_t v[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = base + i < nwords ? (uint32_t)__popcll(bits[base + i]) : 0u;
        s += v[i];
    }
    uint32_t total;
    uint32_t ex = block_excl_scan(s, total);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (base + i < nwords) prefix[base + i] = ex;
        ex += v[i];
    }
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) k_bits_prefix_carry(uint32_t* __restrict__ tile_sums, uint32_t n_tiles,
                                                           uint32_t* __restrict__ total_out) {
    uint32_t carry = 0;
    for (uint32_t b = 0; b < n_tiles; b += 256u) {
        const uint32_t i = b + threadIdx.x;
        uint32_t v = i < n_tiles ? tile_sums[i] : 0u, tot;
        const uint32_t ex = block_excl_scan(v, tot);
        if (i < n_tiles) tile_sums[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ void __launch_bounds__(256) k_bits_prefix_add(uint32_t* __restrict__ prefix,
                                                         const uint32_t* __restrict__ tile_sums, uint32_t nwords) {
    const uint32_t add = tile_sums[blockIdx.x];
    for (uint32_t i = blockIdx.x * (uint32_t)kPrefTile + threadIdx.x; i < (blockIdx.x + 1u) * (uint32_t)kPrefTile;
         i += 256u)
        if (i < nwords) prefix[i] += add;
}

// set bits of `word` below bit b, plus the word's prefix: the rank of voxel v = 64 w + b
__device__ __forceinline__ uint32_t bit_rank(const uint32_t* __restrict__ prefix, uint32_t w, unsigned long long word,
                                             uint32_t b) {
    return prefix[w] + (uint32_t)__popcll(word & ((1ull << b) - 1ull));
}

// one lane = kCandPerThread consecutive (triangle, voxel) candidates, found as k1_candidates
// finds them; a hit in an occupied voxel adds the triangle's three values to that voxel's sums
__global__ void __launch_bounds__(256) k_em_candidates(const TriGeom* __restrict__ geom, const EmFix* __restrict__ fixr,
                                                       const unsigned long long* __restrict__ offs, uint32_t n_tri,
                                                       const unsigned long long* __restrict__ total_p, int n,
                                                       const unsigned long long* __restrict__ occ_bits,
                                                       const uint32_t* __restrict__ occ_prefix,
                                                       const uint32_t* __restrict__ starts,
                                                       unsigned long long* __restrict__ sums) {
    const unsigned long long total = *total_p;
    const unsigned long long c0 = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * kCandPerThread;
    if (c0 >= total) return;
    const unsigned long long bk = c0 / kCandBucket, nbk = (total + kCandBucket - 1) / kCandBucket;
    uint32_t lo = starts[bk], hi = bk + 1 < nbk ? starts[bk + 1] + 1 : n_tri;
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (offs[mid] <= c0) lo = mid; else hi = mid;
    }
    uint32_t t = lo;
    while (t + 1 < n_tri && offs[t + 1] <= c0) ++t;  // skip zero-count triangles
    unsigned long long next = t + 1 < n_tri ? offs[t + 1] : total;
    for (int k = 0; k < kCandPerThread; ++k) {
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
        if (!tri_box_overlap(q, (float)vx + 0.5f, (float)vy + 0.5f, (float)vz + 0.5f)) continue;
        const uint32_t v = (uint32_t)vx + (uint32_t)n * ((uint32_t)vy + (uint32_t)n * (uint32_t)vz);
        const unsigned long long word = occ_bits[v >> 6];
        if (!((word >> (v & 63u)) & 1ull)) continue;             // count(v) == 0: dropped
        unsigned long long* a = sums + 3 * (size_t)bit_rank(occ_prefix, v >> 6, word, v & 63u);
        const EmFix& f = fixr[t];
#pragma unroll
        for (int i = 0; i < 3; ++i) atomicAdd(a + i, (unsigned long long)f.fix[i]);
    }
}

__global__ void __launch_bounds__(256) k_em_mark(const uint32_t* __restrict__ occ_list, uint32_t n_occ,
                                                 const unsigned long long* __restrict__ occ_bits,
                                                 const uint32_t* __restrict__ occ_prefix,
                                                 const long long* __restrict__ sums,
                                                 unsigned long long* __restrict__ em_bits) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_occ; i += gridDim.x * 256u) {
        const uint32_t v = occ_list[i];
        const long long* s = sums + 3 * (size_t)bit_rank(occ_prefix, v >> 6, occ_bits[v >> 6], v & 63u);
        if ((s[0] | s[1] | s[2]) != 0) atomicOr(em_bits + (v >> 6), 1ull << (v & 63u));
    }
}

__global__ void __launch_bounds__(256) k_em_resolve(const uint32_t* __restrict__ occ_list, uint32_t n_occ,
                                                    const unsigned long long* __restrict__ occ_bits,
                                                    const uint32_t* __restrict__ occ_prefix,
                                                    const long long* __restrict__ sums,
                                                    const unsigned long long* __restrict__ em_bits,
                                                    const uint32_t* __restrict__ em_prefix,
                                                    const long long* __restrict__ accum, int packed,
                                                    uint32_t* __restrict__ vox, float4* __restrict__ E) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_occ; i += gridDim.x * 256u) {
        const uint32_t v = occ_list[i];
        const unsigned long long ew = em_bits[v >> 6];
        if (!((ew >> (v & 63u)) & 1ull)) continue;
        const long long* s = sums + 3 * (size_t)bit_rank(occ_prefix, v >> 6, occ_bits[v >> 6], v & 63u);
        // K1's hit count of the voxel: word 3 of a packed record, word 6 of a seven-atomic one
        const unsigned long long cnt = (unsigned long long)accum[8 * (size_t)v + (packed ? 3 : 6)];
        const double den = (double)cnt * VCT_FIXED_ONE_D;
        const uint32_t r = bit_rank(em_prefix, v >> 6, ew, v & 63u);
        vox[r] = v;
        E[r] = make_float4((float)((double)s[0] / den), (float)((double)s[1] / den), (float)((double)s[2] / den), 1.0f);
    }
}

// level 0 += scale * E: the product, then the add (no fma: -ffp-contract=off); alpha untouched
__global__ void __launch_bounds__(256) k_em_add(const uint32_t* __restrict__ vox, const uint32_t* __restrict__ count,
                                                const float4* __restrict__ E, float scale, float4* __restrict__ r0,
                                                uint32_t n) {
    const uint32_t cnt = *count;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < cnt; i += gridDim.x * 256u) {
        const float4 e = E[i];
        float4* dst = r0 + l0_texel(vox[i], n);
        float4 L = *dst;
        L.x = L.x + scale * e.x;
        L.y = L.y + scale * e.y;
        L.z = L.z + scale * e.z;
        *dst = L;
    }
}

// ---- composite + present with the emission term -----------------------------------------
struct CompEK {
    const float4 *pos, *nrm, *alb, *diff, *spec;
    const float* vis;                      // VIS: [n_lights][h][w]
    const unsigned long long* bits;        // !VIS: K1's occupancy, for the walk
    const unsigned long long* em_bits;     // EM
    const uint32_t* em_prefix;
    const float4* em_E;
    int n, w, h;
    float g0x, g0y, g0z, inv_h, h2, scale;
    uint32_t n_lights;
    float4* lin;
    uint32_t* rgba8;
};

// VIS: V read from the vis plane (ks_composite), else walked (kl_composite); EM: the grid may
// hold an emissive voxel and scale != 0 (otherwise the other composites' arithmetic, unchanged)
template <bool VIS, bool EM>
__global__ void __launch_bounds__(256) k_em_composite(const CompEK k, const LightSet set) {
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
        else vis = dda_lim(k.bits, k.n, qx, qy, qz, lx, ly, lz, t_lim);
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
struct DevTmp {   // a staging buffer of the host form, freed on every exit
    void* p = nullptr;
    ~DevTmp() { if (p) (void)hipFree(p); }
};

// scale of vct_inject_emission / vct_composite_emissive_device: finite, sign bit clear,
// <= VCT_EMISSION_SCALE_LIMIT
const char* check_scale(float scale) {
    if (!std::isfinite(scale)) return "non-finite scale";
    if (std::signbit(scale)) return "negative scale";
    if (scale > VCT_EMISSION_SCALE_LIMIT) return "scale above VCT_EMISSION_SCALE_LIMIT";
    return nullptr;
}

// popc prefix of `bits` into `prefix`, the total into *total_out (all device); tiles: scratch
void launch_bits_prefix(hipStream_t s, const unsigned long long* bits, uint32_t nwords, uint32_t* prefix,
                        uint32_t* tiles, uint32_t* total_out) {
    const uint32_t n_tiles = (nwords + kPrefTile - 1) / kPrefTile;
    hipLaunchKernelGGL(k_bits_prefix_tiles, dim3(n_tiles), dim3(256), 0, s, bits, nwords, prefix, tiles);
    hipLaunchKernelGGL(k_bits_prefix_carry, dim3(1), dim3(256), 0, s, tiles, n_tiles, total_out);
    hipLaunchKernelGGL(k_bits_prefix_add, dim3(n_tiles), dim3(256), 0, s, prefix, (const uint32_t*)tiles, nwords);
}

template <typename T>
hipError_t regrow(T*& p, size_t count) {
    if (p) (void)hipFree(p);
    p = nullptr;
    return hipMalloc((void**)&p, count * sizeof(T));
}

// The emission grid of the current voxelization from device-resident emitter geometry.
// Waits for the ctx stream once (candidate total, occupied voxels, error word).
vct_status emission_build(vct_ctx* c, const void* d_verts, uint32_t stride, uint32_t n_verts, const uint32_t* d_idx,
                          uint32_t n_tri, const uint32_t* d_mat, const float4* d_ke, uint32_t n_mat) {
    Grid& g = c->grid;
    Emission& em = c->em;
    hipStream_t s = c->stream;
    const size_t nv = (size_t)g.n * g.n * g.n;
    const uint32_t nwords = (uint32_t)(nv / 64);
    const uint32_t n_ptiles = (nwords + kPrefTile - 1) / kPrefTile;
    hipError_t e;
    if (!em.bits) {
        if ((e = hipMalloc((void**)&em.bits, (size_t)nwords * 8)) != hipSuccess) return lhip(c, e, "emission: bits");
        if ((e = hipMalloc((void**)&em.prefix, (size_t)nwords * 4)) != hipSuccess) return lhip(c, e, "emission: prefix");
        if ((e = hipMalloc((void**)&em.count, 16)) != hipSuccess) return lhip(c, e, "emission: count");
    }
    // triangle temps: geom | fix | counts | offsets | tile sums | head
    const uint32_t n_tiles = (n_tri + kScanTile - 1) / kScanTile;
    const size_t off_geom = 0;
    const size_t off_fix = off_geom + sizeof(TriGeom) * (size_t)n_tri;
    const size_t off_cnt = off_fix + sizeof(EmFix) * (size_t)n_tri;
    const size_t off_offs = off_cnt + 8 * (size_t)n_tri;
    const size_t off_tiles = off_offs + 8 * (size_t)n_tri;
    const size_t off_head = off_tiles + 8 * (size_t)(n_tiles + 1);
    void* sp;
    if ((e = scratch_get(c, kSlotTri, off_head + sizeof(EmHead), &sp)) != hipSuccess) return lhip(c, e, "emission: scratch");
    char* base = (char*)sp;
    TriGeom* geom = (TriGeom*)(base + off_geom);
    EmFix* fix = (EmFix*)(base + off_fix);
    unsigned long long* cnt = (unsigned long long*)(base + off_cnt);
    unsigned long long* offs = (unsigned long long*)(base + off_offs);
    unsigned long long* tiles = (unsigned long long*)(base + off_tiles);
    EmHead* head = (EmHead*)(base + off_head);
    // occupancy ranks: prefix | tile sums
    void* rp;
    if ((e = scratch_get(c, kSlotRank, ((size_t)nwords + n_ptiles) * 4, &rp)) != hipSuccess)
        return lhip(c, e, "emission: scratch");
    uint32_t* occ_prefix = (uint32_t*)rp;
    uint32_t* ptiles = occ_prefix + nwords;

    if ((e = hipMemsetAsync(head, 0, sizeof(EmHead), s)) != hipSuccess) return lhip(c, e, "emission: memset");
    if (n_tri > 0) {
        hipLaunchKernelGGL(k_em_setup, dim3((n_tri + 255) / 256), dim3(256), 0, s, (const char*)d_verts, stride, n_verts,
                           d_idx, n_tri, d_mat, d_ke, n_mat, (int)g.n, g.g0[0], g.g0[1], g.g0[2], g.inv_h, geom, fix,
                           cnt, &head->err);
        hipLaunchKernelGGL(k_scan_tiles, dim3(n_tiles), dim3(kScanBlock), 0, s, cnt, offs, tiles, n_tri);
        hipLaunchKernelGGL(k_scan_carry, dim3(1), dim3(kScanBlock), 0, s, tiles, n_tiles, &head->total);
        hipLaunchKernelGGL(k_scan_add, dim3(n_tiles), dim3(kScanBlock), 0, s, offs, tiles, n_tri);
    }
    launch_bits_prefix(s, g.occ_bits, nwords, occ_prefix, ptiles, &head->n_occ);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "emission: setup");
    EmHead h{};
    if ((e = hipMemcpyAsync(&h, head, sizeof h, hipMemcpyDeviceToHost, s)) != hipSuccess) return lhip(c, e, "emission: read back");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return lhip(c, e, "emission: sync");
    if (h.err & kEmErrKe)
        return lfail(c, VCT_EINVAL, "voxelize_emission: material_ke4: Ke not finite, negative or >= 32768");
    if (h.err & kEmErrIndex) return lfail(c, VCT_EINVAL, "voxelize_emission: vertex or material index out of range");
    if ((size_t)h.n_occ > nv) return lfail(c, VCT_EDEVICE, "voxelize_emission: occupancy count out of range");

    if (h.total > 0 && h.n_occ > 0) {
        if (em.cap < h.n_occ) {   // (the stream is idle: nothing reads the old arrays)
            em.cap = 0;
            if ((e = regrow(em.sums, (size_t)h.n_occ * 3)) != hipSuccess) return lhip(c, e, "emission: sums");
            if ((e = regrow(em.vox, (size_t)h.n_occ)) != hipSuccess) return lhip(c, e, "emission: voxel list");
            if ((e = regrow(em.E, (size_t)h.n_occ)) != hipSuccess) return lhip(c, e, "emission: E");
            em.cap = h.n_occ;
        }
        const unsigned long long threads = (h.total + kCandPerThread - 1) / kCandPerThread;
        const unsigned long long blocks = (threads + 255) / 256;
        if (blocks > 0x7fffffffull) return lfail(c, VCT_EINVAL, "voxelize_emission: too many candidates");
        const unsigned long long nbk = (h.total + kCandBucket - 1) / kCandBucket;
        void* bp;
        if ((e = scratch_get(c, kSlotBuckets, (size_t)nbk * 4, &bp)) != hipSuccess) return lhip(c, e, "emission: scratch");
        uint32_t* starts = (uint32_t*)bp;
        if ((e = hipMemsetAsync(em.sums, 0, (size_t)h.n_occ * 24, s)) != hipSuccess) return lhip(c, e, "emission: memset");
        if ((e = hipMemsetAsync(em.bits, 0, (size_t)nwords * 8, s)) != hipSuccess) return lhip(c, e, "emission: memset");
        hipLaunchKernelGGL(k1_bucket_starts, dim3((n_tri + 255) / 256), dim3(256), 0, s, offs, n_tri, &head->total, starts);
        hipLaunchKernelGGL(k_em_candidates, dim3((uint32_t)blocks), dim3(256), 0, s, geom, fix, offs, n_tri, &head->total,
                           (int)g.n, g.occ_bits, occ_prefix, starts, (unsigned long long*)em.sums);
        const uint32_t lb = std::min<uint32_t>((h.n_occ + 255u) / 256u, 4096u);
        hipLaunchKernelGGL(k_em_mark, dim3(lb), dim3(256), 0, s, g.occ_list, h.n_occ, g.occ_bits, occ_prefix, em.sums,
                           em.bits);
        launch_bits_prefix(s, em.bits, nwords, em.prefix, ptiles, em.count);
        hipLaunchKernelGGL(k_em_resolve, dim3(lb), dim3(256), 0, s, g.occ_list, h.n_occ, g.occ_bits, occ_prefix, em.sums,
                           em.bits, em.prefix, (const long long*)g.accum, g.accum_packed ? 1 : 0, em.vox, em.E);
        if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "emission: build");
        em.maybe = true;
        em.n_host = -1;
    } else {
        em.maybe = false;     // no candidate or no occupied voxel: empty, nothing launched
        em.n_host = 0;
    }
    em.epoch = c->grid_epoch;
    em.built = true;
    return VCT_OK;
}

vct_status emission_args(vct_ctx* c, const void* verts, uint32_t stride, uint32_t n_idx, const uint32_t* idx,
                         const float* ke4) {
    c->em.built = false;   // whatever goes wrong below, the emission grid is empty afterwards
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "voxelize_emission before voxelize");
    if (n_idx % 3 != 0) return lfail(c, VCT_EINVAL, "voxelize_emission: n_idx must be a multiple of 3");
    if (n_idx > 0 && (!verts || !idx)) return lfail(c, VCT_EINVAL, "voxelize_emission: null vertex or index array");
    if (stride < 12 || stride % 4 != 0)
        return lfail(c, VCT_EINVAL, "voxelize_emission: vertex_stride < 12 or not a multiple of 4");
    if (!ke4) return lfail(c, VCT_EINVAL, "voxelize_emission: NULL material_ke4");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    return VCT_OK;
}

// the count of emissive voxels, read back once per build (waits for the ctx stream)
vct_status emission_count(vct_ctx* c, uint32_t* out) {
    Emission& em = c->em;
    *out = 0;
    if (!emission_live(c)) return VCT_OK;
    if (em.n_host < 0) {
        hipError_t e = hipSetDevice(c->device);
        if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
        uint32_t n = 0;
        if ((e = hipMemcpyAsync(&n, em.count, 4, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
            return lhip(c, e, "emission: read back");
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return lhip(c, e, "emission: sync");
        if ((size_t)n > em.cap) return lfail(c, VCT_EDEVICE, "emission: count out of range");
        em.n_host = n;
    }
    *out = (uint32_t)em.n_host;
    return VCT_OK;
}

}  // namespace

void emission_free(vct_ctx* c) {
    Emission& em = c->em;
    for (void* p : {(void*)em.bits, (void*)em.prefix, (void*)em.sums, (void*)em.vox, (void*)em.E, (void*)em.count})
        if (p) (void)hipFree(p);
    em = Emission{};
}

}  // namespace vct

using namespace vct;

extern "C" vct_status vct_voxelize_emission_device(vct_ctx* c, const void* verts, uint32_t stride, uint32_t n_verts,
                                                   const uint32_t* idx, uint32_t n_idx, const uint32_t* tri_mat,
                                                   const float* ke4, uint32_t n_mat) {
    if (!c) return VCT_EINVAL;
    vct_status st = emission_args(c, verts, stride, n_idx, idx, ke4);
    if (st != VCT_OK) return st;
    if (((uintptr_t)ke4 & 15) || ((uintptr_t)verts & 3) || ((uintptr_t)idx & 3) || ((uintptr_t)tri_mat & 3))
        return lfail(c, VCT_EINVAL, "voxelize_emission: material_ke4 must be 16-byte, verts, idx and tri_material "
                                    "4-byte aligned");
    return emission_build(c, verts, stride, n_verts, idx, n_idx / 3, tri_mat, (const float4*)ke4, n_mat);
}

extern "C" vct_status vct_voxelize_emission(vct_ctx* c, const void* verts, uint32_t stride, uint32_t n_verts,
                                            const uint32_t* idx, uint32_t n_idx, const uint32_t* tri_mat,
                                            const float* ke4, uint32_t n_mat) {
    if (!c) return VCT_EINVAL;
    vct_status st = emission_args(c, verts, stride, n_idx, idx, ke4);
    if (st != VCT_OK) return st;
    const uint32_t n_tri = n_idx / 3;
    // the Ke rule on the host, before any launch: the Ke of every material a triangle uses
    // (an out-of-range material index is the setup kernel's to report)
    for (uint32_t t = 0; t < n_tri; ++t) {
        const uint32_t m = tri_mat ? tri_mat[t] : 0u;
        if (m >= n_mat) continue;
        const float* k = ke4 + 4 * (size_t)m;
        if (!(ke_legal(k[0]) && ke_legal(k[1]) && ke_legal(k[2])))
            return lfail(c, VCT_EINVAL, "voxelize_emission: material_ke4[" + std::to_string(m) +
                                            "]: Ke not finite, negative or >= 32768");
    }
    DevTmp dv, di, dm, dk;
    const size_t vbytes = (size_t)stride * n_verts;
    hipError_t e;
    if (vbytes && (e = hipMalloc(&dv.p, vbytes)) != hipSuccess) return lhip(c, e, "hipMalloc verts");
    if (n_idx && (e = hipMalloc(&di.p, (size_t)n_idx * 4)) != hipSuccess) return lhip(c, e, "hipMalloc idx");
    if (tri_mat && n_tri && (e = hipMalloc(&dm.p, (size_t)n_tri * 4)) != hipSuccess) return lhip(c, e, "hipMalloc mat");
    if ((e = hipMalloc(&dk.p, (size_t)(n_mat ? n_mat : 1) * 16)) != hipSuccess) return lhip(c, e, "hipMalloc ke");
    if (vbytes && (e = hipMemcpyAsync(dv.p, verts, vbytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
        return lhip(c, e, "upload verts");
    if (n_idx && (e = hipMemcpyAsync(di.p, idx, (size_t)n_idx * 4, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
        return lhip(c, e, "upload idx");
    if (dm.p && (e = hipMemcpyAsync(dm.p, tri_mat, (size_t)n_tri * 4, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
        return lhip(c, e, "upload mat");
    if (n_mat && (e = hipMemcpyAsync(dk.p, ke4, (size_t)n_mat * 16, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
        return lhip(c, e, "upload ke");
    st = emission_build(c, dv.p, stride, n_verts, (const uint32_t*)di.p, n_tri, (const uint32_t*)dm.p,
                        (const float4*)dk.p, n_mat);
    // the staging buffers are freed on return: everything that reads them must have run
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess && st == VCT_OK) st = lhip(c, e, "emission: sync");
    return st;
}

extern "C" vct_status vct_emission_voxels(vct_ctx* c, uint32_t* n_emissive) {
    if (!c || !n_emissive) return c ? lfail(c, VCT_EINVAL, "emission_voxels: null output") : VCT_EINVAL;
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "emission_voxels before voxelize");
    return emission_count(c, n_emissive);
}

extern "C" vct_status vct_download_emission(vct_ctx* c, float* host_rgba) {
    if (!c || !host_rgba) return c ? lfail(c, VCT_EINVAL, "download_emission: null output") : VCT_EINVAL;
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "download_emission before voxelize");
    const size_t nv = (size_t)c->grid.n * c->grid.n * c->grid.n;
    std::memset(host_rgba, 0, nv * 16);
    uint32_t n = 0;
    vct_status st = emission_count(c, &n);
    if (st != VCT_OK || n == 0) return st;
    std::vector<uint32_t> vox(n);
    std::vector<float> E((size_t)n * 4);
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    if ((e = hipMemcpyAsync(vox.data(), c->em.vox, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipMemcpyAsync(E.data(), c->em.E, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return lhip(c, e, "download_emission");
    for (uint32_t i = 0; i < n; ++i) {
        if (vox[i] >= nv) return lfail(c, VCT_EDEVICE, "download_emission: voxel index out of range");
        std::memcpy(host_rgba + 4 * (size_t)vox[i], E.data() + 4 * (size_t)i, 16);
    }
    return VCT_OK;
}

extern "C" vct_status vct_inject_emission(vct_ctx* c, float scale) {
    if (!c) return VCT_EINVAL;
    Grid& g = c->grid;
    if (const char* bad = check_scale(scale)) return lfail(c, VCT_EINVAL, std::string("inject_emission: ") + bad);
    if (!g.voxelized) return lfail(c, VCT_ESTATE, "inject_emission before voxelize");
    if (!g.injected) return lfail(c, VCT_ESTATE, "inject_emission without a level 0 (inject or upload one first)");
    if (g.emitted)
        return lfail(c, VCT_ESTATE, "inject_emission twice on one level 0 (inject or upload a new one first)");
    if (g.bounced)
        return lfail(c, VCT_ESTATE, "inject_emission after inject_bounces on this level 0 (the bounce's level 0 must "
                                    "already hold the emission)");
    if (!emission_live(c)) return VCT_OK;   // an empty emission grid: nothing to add, nothing changes
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    const Emission& em = c->em;
    const uint32_t blocks = (uint32_t)std::min<size_t>((em.cap + 255) / 256, 2048);
    hipLaunchKernelGGL(k_em_add, dim3(blocks), dim3(256), 0, c->stream, (const uint32_t*)em.vox,
                       (const uint32_t*)em.count, (const float4*)em.E, scale, g.pyr, g.n);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "inject_emission");
    g.emitted = true;
    g.mipped = false;
    g.l0_on_peers = false;   // device 0 added: the next vct_build_mips copies level 0 to the other devices
    return VCT_OK;
}

extern "C" vct_status vct_composite_emissive_device(vct_ctx* c, const float* pos4, const float* nrm4, const float* alb4,
                                                    const float* diffuse4, const float* spec4, uint32_t w, uint32_t h,
                                                    const vct_light* lights, uint32_t n_lights, const float* vis,
                                                    float scale, float* out_linear4, uint32_t* out_rgba8) {
    if (!c || !pos4 || !nrm4 || !alb4 || !diffuse4 || !spec4 || w == 0 || h == 0) return VCT_EINVAL;
    if (!out_linear4 && !out_rgba8) return lfail(c, VCT_EINVAL, "composite: no output");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "composite: frame too large");
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "composite before voxelize");
    for (const void* p : {(const void*)pos4, (const void*)nrm4, (const void*)alb4, (const void*)diffuse4,
                          (const void*)spec4, (const void*)out_linear4})
        if (((uintptr_t)p & 15u) != 0) return lfail(c, VCT_EINVAL, "composite: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)out_rgba8 & 3u) != 0) return lfail(c, VCT_EINVAL, "composite: rgba8 buffer must be 4-byte aligned");
    if (((uintptr_t)vis & 3u) != 0) return lfail(c, VCT_EINVAL, "composite_emissive: vis must be 4-byte aligned");
    if (const char* bad = check_scale(scale)) return lfail(c, VCT_EINVAL, std::string("composite_emissive: ") + bad);
    LightSet set;
    std::memset(&set, 0, sizeof set);
    vct_status st = prepare_list(c, "composite_emissive", lights, n_lights, set.l);
    if (st != VCT_OK) return st;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    const Grid& g = c->grid;
    const Emission& em = c->em;
    CompEK k;
    std::memset(&k, 0, sizeof k);
    k.pos = (const float4*)pos4; k.nrm = (const float4*)nrm4; k.alb = (const float4*)alb4;
    k.diff = (const float4*)diffuse4; k.spec = (const float4*)spec4;
    k.vis = vis;
    k.bits = g.occ_bits;
    k.em_bits = em.bits; k.em_prefix = em.prefix; k.em_E = em.E;
    k.n = (int)g.n; k.w = (int)w; k.h = (int)h;
    k.g0x = g.g0[0]; k.g0y = g.g0[1]; k.g0z = g.g0[2]; k.inv_h = g.inv_h; k.h2 = grid_h2(g);
    k.scale = scale;
    k.n_lights = n_lights;
    k.lin = (float4*)out_linear4; k.rgba8 = out_rgba8;
    const bool emit = scale != 0.0f && emission_live(c);
    const dim3 grid((w * h + 255) / 256), block(256);
    if (vis) {
        if (emit) hipLaunchKernelGGL((k_em_composite<true, true>), grid, block, 0, c->stream, k, set);
        else hipLaunchKernelGGL((k_em_composite<true, false>), grid, block, 0, c->stream, k, set);
    } else {
        if (emit) hipLaunchKernelGGL((k_em_composite<false, true>), grid, block, 0, c->stream, k, set);
        else hipLaunchKernelGGL((k_em_composite<false, false>), grid, block, 0, c->stream, k, set);
    }
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "composite_emissive");
    return VCT_OK;
}
