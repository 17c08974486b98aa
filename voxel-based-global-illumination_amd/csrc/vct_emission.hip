// vct_emission.hip — emissive surfaces (include/vct_emission.h; the arithmetic is
// include/vct_spec.h "emissive surfaces"): the emission grid E of a voxelization, its add
// into level 0, and the entry point of the composite that shows it.
//
// The build is a K1-shaped pass over the emitter triangles (vct_voxel_sat.h: K1's triangle
// setup pieces, scan, bucket table and candidate walk; this unit keeps the Ke rule, its three
// values and what a hit does):
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
// The composite is kl_composite<VIS, EM> (vct_lights.hip), whose EM form adds scale * E of the
// pixel's voxel; vct_composite_emissive_device here keeps its own rule (vis optional, the scale).
// Memory: the sums and the compact arrays are sized by the occupied voxels (44 bytes each);
// only the bit and prefix words are sized by the grid (3 n^3 / 16 bytes).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include "vct_internal.h"
#include "vct_voxel_sat.h"

namespace vct {
namespace {

constexpr int kEmErrIndex = 1, kEmErrKe = 2;
constexpr int kSlotRank = 11;   // vct_ctx::scratch (1 and 7 as K1 uses them: tri_temps, launch_bucket_starts)

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
    const uint32_t m = mat ? mat[t] : 0u;
    uint32_t vi[3];
    float p[3][3], q[3][3];
    if (m >= n_mat || !load_tri(verts, stride, n_verts, idx, t, g0x, g0y, g0z, inv_h, vi, p, q)) {
        atomicOr(err, kEmErrIndex);
        reject_tri(geom, counts, t);
        return;
    }
    const float4 k4 = ke[m];
    if (!(ke_legal(k4.x) && ke_legal(k4.y) && ke_legal(k4.z))) {
        atomicOr(err, kEmErrKe);
        reject_tri(geom, counts, t);
        return;
    }
    EmFix f;
    f.fix[0] = (long long)roundf(k4.x * VCT_FIXED_ONE);
    f.fix[1] = (long long)roundf(k4.y * VCT_FIXED_ONE);
    f.fix[2] = (long long)roundf(k4.z * VCT_FIXED_ONE);
    f.pad = 0;
    // K1 input rule: a non-finite q is skipped; a triangle that emits nothing has no candidates
    if (!tri_finite(q) || (f.fix[0] | f.fix[1] | f.fix[2]) == 0) {
        reject_tri(geom, counts, t);
        return;
    }
    TriGeom g;
    counts[t] = tri_range(q, n, g);
    geom[t] = g;
    fixo[t] = f;
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
    const uint32_t t0 = find_tri_bucketed(offs, starts, n_tri, total, c0);
    for_each_hit<kCandPerThread>(geom, offs, n_tri, total, c0, t0,
                                 [&](uint32_t t, int vx, int vy, int vz, const float*) __attribute__((always_inline)) {
        const uint32_t v = (uint32_t)vx + (uint32_t)n * ((uint32_t)vy + (uint32_t)n * (uint32_t)vz);
        const unsigned long long word = occ_bits[v >> 6];
        if (!((word >> (v & 63u)) & 1ull)) return;               // count(v) == 0: dropped
        unsigned long long* a = sums + 3 * (size_t)bit_rank(occ_prefix, v >> 6, word, v & 63u);
        const EmFix& f = fixr[t];
#pragma unroll
        for (int i = 0; i < 3; ++i) atomicAdd(a + i, (unsigned long long)f.fix[i]);
    });
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

// ---- host side --------------------------------------------------------------------------
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
    TriTemps tt;
    if ((e = tri_temps(c, n_tri, sizeof(EmFix), 0, tt)) != hipSuccess) return lhip(c, e, "emission: scratch");
    TriGeom* geom = tt.geom;
    EmFix* fix = (EmFix*)tt.fix;
    unsigned long long* offs = tt.offs;
    EmHead* head = (EmHead*)tt.head;
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
                           tt.counts, &head->err);
        launch_count_scan(s, tt.counts, offs, tt.tiles, n_tri, &head->total);
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
        uint32_t blocks;
        uint32_t* starts;
        e = launch_bucket_starts(c, offs, n_tri, &head->total, h.total, &blocks, &starts);
        if (e == hipErrorInvalidValue) return lfail(c, VCT_EINVAL, "voxelize_emission: too many candidates");
        if (e != hipSuccess) return lhip(c, e, "emission: scratch");
        if ((e = hipMemsetAsync(em.sums, 0, (size_t)h.n_occ * 24, s)) != hipSuccess) return lhip(c, e, "emission: memset");
        if ((e = hipMemsetAsync(em.bits, 0, (size_t)nwords * 8, s)) != hipSuccess) return lhip(c, e, "emission: memset");
        hipLaunchKernelGGL(k_em_candidates, dim3(blocks), dim3(256), 0, s, geom, fix, offs, n_tri, &head->total,
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
    MeshStage ms;
    if ((st = stage_mesh(c, ms, verts, (size_t)stride * n_verts, idx, n_idx, tri_mat, ke4, "ke", nullptr, n_mat)) != VCT_OK)
        return st;
    st = emission_build(c, ms.verts.p, stride, n_verts, (const uint32_t*)ms.idx.p, n_tri, (const uint32_t*)ms.mat.p,
                        (const float4*)ms.mats.p, n_mat);
    hipError_t e;
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
    // vis is optional (NULL: V is walked); the term is live when the grid may hold an emissive voxel
    CompositeForm form;
    form.vis = vis;
    form.read_vis = vis != nullptr;
    form.scale = scale;
    form.emit = c && scale != 0.0f && emission_live(c);
    form.own_error = ((uintptr_t)vis & 3u) != 0 ? "vis must be 4-byte aligned" : check_scale(scale);
    return composite_light_list(c, "composite_emissive", pos4, nrm4, alb4, diffuse4, spec4, w, h, lights, n_lights, form,
                                out_linear4, out_rgba8);
}
