// vct_cutout.hip — alpha-cutout materials (include/vct_cutout.h; vct_spec.h "cutouts"):
//  * k1_tri_setup_cutout: K1's triangle setup (vct_voxelize.hip k1_tri_setup, from the shared
//    pieces of vct_voxel_sat.h) with the material's mask in the records: the mask word in
//    TriFix::pad, the cutoff in TriUV::pad[0], the TexCoords of every masked triangle kept, in
//    Mesh::uv too, and the word pair the G-buffer pass reads in Cutout::tri;
//  * k1_candidates_cutout: K1's candidates kernel over for_each_hit; the hit functor samples the
//    mask before any atomic and returns when the point is not covered.  A mask that is the
//    diffuse map is fetched once for both;
//  * k_bin_raster_cutout: k_bin_raster's candidate loop over the bins of vct_frame.hip's binning,
//    unchanged, with a "masked" bit beside the staged id in LDS.  The mask is sampled only for a
//    candidate that would win now (t < best, or t == best with a lower id); a rejected one leaves
//    the winner as it was, so the result is the minimum over the accepted candidates, ties to
//    the lower id, whatever order k_bin_fill left in the bin.  One kernel for the flat and the
//    shaded records (the writer is a template parameter).
#include <cmath>
#include <cstring>
#include "vct_internal.h"
#include "vct_voxel_sat.h"
#include "vct_view.h"
#include "vct_gbuffer.h"
#include "vct_shaded.h"

namespace vct {
namespace {

constexpr uint32_t kOpaque = 0xFFFFFFFFu;   // a mask word: no mask

// M_channel(u, v) >= cutoff for the mask word `mw` (4 * map + channel)
__device__ __forceinline__ bool covered(const uint32_t* __restrict__ texels, const TexDesc* __restrict__ tdesc,
                                        uint32_t mw, float cutoff, float u, float v) {
    const TexTap q = tex_tap(texels, tdesc[mw >> 2], u, v);
    return tex_channel(q, mw & 3u) >= cutoff;
}

// ---- K1 ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k1_tri_setup_cutout(K1SetupArgs a, const vct_cutout* __restrict__ cut,
                                                           uint2* __restrict__ cut_tri) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_tri) return;
    TriGeom* geom = (TriGeom*)a.geom;
    const uint32_t m = a.mat ? a.mat[t] : 0u;
    // the material's diffuse map and mask; a material index past the tables -> error
    const int32_t tex = (a.map && m < a.n_mat) ? a.map[m] : -1;
    const bool mat_ok = !(m >= a.n_mat || tex < -1 || (tex >= 0 && (uint32_t)tex >= a.n_tex));
    uint32_t mw = kOpaque;
    float cutoff = 1.0f;
    if (mat_ok) {   // (the host has checked every entry against the texture set)
        const vct_cutout ct = cut[m];
        if (ct.map >= 0) { mw = 4u * (uint32_t)ct.map + ct.channel; cutoff = ct.cutoff; }
    }
    uint32_t vi[3];
    float p[3][3], q[3][3];
    if (!mat_ok || !load_tri(a.verts, a.stride, a.n_verts, a.idx, t, a.g0x, a.g0y, a.g0z, a.inv_h, vi, p, q)) {
        atomicOr(a.err, kK1ErrIndex);
        reject_tri(geom, a.counts, t);
        return;
    }
    const float4 alb = a.kd ? a.kd[m] : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const bool kd_ok = kd_legal(alb.x, alb.y, alb.z);
    const bool uvs = tex >= 0 || mw != kOpaque;
    if (!kd_ok || !tri_finite(q)) {   // K1 skips it: a zero triangle for the G-buffer passes, never hit
        if (!kd_ok) atomicOr(a.err, kK1ErrKd);
        reject_tri(geom, a.counts, t);
        const float z[3] = {0.0f, 0.0f, 0.0f};
        store_mesh_tri(a.mesh_tri, t, z, z, z, alb, -1);
        const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (uvs) { a.mesh_uv[2 * t + 0] = z4; a.mesh_uv[2 * t + 1] = z4; }
        cut_tri[t] = make_uint2(kOpaque, 0u);
        return;
    }
    TriGeom g;
    TriFix f;
    float e1[3], e2[3];
    face_fix(p, alb, f.fix, e1, e2);
    f.tex = tex;
    f.pad = mw == kOpaque ? -1ll : (long long)mw;
    fix_maxabs(f.fix, a.maxabs);
    if (uvs) {
        TriUV r;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* src = (const float*)(a.verts + (size_t)vi[k] * a.stride + a.uv_offset);
            r.uv[2 * k] = src[0];
            r.uv[2 * k + 1] = src[1];
        }
        r.kd[0] = alb.x; r.kd[1] = alb.y; r.kd[2] = alb.z;
        r.pad[0] = __float_as_uint(cutoff);
        r.pad[1] = r.pad[2] = 0;
        ((TriUV*)a.tuv)[t] = r;
        a.mesh_uv[2 * t + 0] = make_float4(r.uv[0], r.uv[1], r.uv[2], r.uv[3]);
        a.mesh_uv[2 * t + 1] = make_float4(r.uv[4], r.uv[5], 0.0f, 0.0f);
    }
    a.counts[t] = tri_range(q, a.n, g);
    geom[t] = g;
    ((TriFix*)a.fix)[t] = f;
    store_mesh_tri(a.mesh_tri, t, p[0], e1, e2, alb, tex);
    cut_tri[t] = make_uint2(mw, __float_as_uint(cutoff));
}

// k1_candidates (vct_voxelize.hip) with the coverage test in front of the atomics
template <bool PACKED>
__global__ void __launch_bounds__(256) k1_candidates_cutout(const TriGeom* __restrict__ geom,
                                                            const TriFix* __restrict__ fixr,
                                                            const unsigned long long* __restrict__ offs,
                                                            uint32_t n_tri, const unsigned long long* __restrict__ total_p,
                                                            int n, long long* __restrict__ accum,
                                                            unsigned long long* __restrict__ occ_bits,
                                                            const uint32_t* __restrict__ starts,
                                                            const TriUV* __restrict__ tuv,
                                                            const uint32_t* __restrict__ texels,
                                                            const TexDesc* __restrict__ tdesc) {
    const unsigned long long total = *total_p;
    const unsigned long long c0 = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * kCandPerThread;
    if (c0 >= total) return;
    const uint32_t t0 = find_tri_bucketed(offs, starts, n_tri, total, c0);
    for_each_hit<kCandPerThread>(geom, offs, n_tri, total, c0, t0,
                                 [&](uint32_t t, int vx, int vy, int vz, const float* q) __attribute__((always_inline)) {
        const TriFix& f = fixr[t];
        long long fa[3] = {f.fix[0], f.fix[1], f.fix[2]};
        const long long mask = f.pad;
        if (f.tex >= 0 || mask >= 0) {   // the point of the pair: the voxel centre's projection
            const TriUV r = tuv[t];
            float b1, b2, u, w;
            tri_bary(q, (float)vx + 0.5f, (float)vy + 0.5f, (float)vz + 0.5f, b1, b2);
            tri_uv(r.uv, b1, b2, u, w);
            TexTap tap;
            bool have = false;   // tap holds the diffuse map's texels
            if (mask >= 0) {
                const uint32_t mw = (uint32_t)mask;
                tap = tex_tap(texels, tdesc[mw >> 2], u, w);
                if (!(tex_channel(tap, mw & 3u) >= __uint_as_float(r.pad[0]))) return;   // not covered: adds nothing
                have = (long long)(mw >> 2) == f.tex;
            }
            if (f.tex >= 0) {   // albedo = Kd x T(uv), as k1_candidates
                if (!have) tap = tex_tap(texels, tdesc[f.tex], u, w);
                fa[0] = (long long)roundf((r.kd[0] * tex_channel(tap, 0u)) * VCT_FIXED_ONE);
                fa[1] = (long long)roundf((r.kd[1] * tex_channel(tap, 1u)) * VCT_FIXED_ONE);
                fa[2] = (long long)roundf((r.kd[2] * tex_channel(tap, 2u)) * VCT_FIXED_ONE);
            }
        }
        size_t v = (size_t)vx + (size_t)n * ((size_t)vy + (size_t)n * (size_t)vz);
        unsigned long long* a = (unsigned long long*)(accum + 8 * v);
        if constexpr (PACKED) {
            atomicAdd(a + 0, (unsigned long long)fa[0] + ((unsigned long long)fa[1] << 32));
            atomicAdd(a + 1, (unsigned long long)fa[2] + ((unsigned long long)f.fix[3] << 32));
            atomicAdd(a + 2, (unsigned long long)f.fix[4] + ((unsigned long long)f.fix[5] << 32));
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) atomicAdd(a + i, (unsigned long long)fa[i]);
#pragma unroll
            for (int i = 3; i < 6; ++i) atomicAdd(a + i, (unsigned long long)f.fix[i]);
        }
        if (atomicAdd(a + (PACKED ? 3 : 6), 1ull) == 0ull) atomicOr(occ_bits + (v >> 6), 1ull << (v & 63));   // first hit
    });
}

// ---- the G-buffer pass --------------------------------------------------------------------------
struct CutK {
    const uint2* tri;   // [n_cut] mask word, cutoff bits (NULL: no cutout mesh)
    uint32_t n_cut;     // triangles past it (the dynamic layer) are opaque
};

constexpr uint32_t kMaskedBit = 0x80000000u;   // beside the staged id (a triangle id is an int >= 0)

// The occupancy of the two passes it stands in for (vct_shading.hip has the register figures)
template <bool SHADED>
__global__ void __launch_bounds__(256, 8) k_bin_raster_cutout(BinK k, ShadeK s, CutK c) {
    __shared__ float4 sh[kRayChunk * 3];
    __shared__ uint32_t sid[kRayChunk];
    const RayK& r = k.r;
    const int tile = (int)blockIdx.x;
    const int x = (tile % k.tiles_x) * kGT + (int)(threadIdx.x & 15);
    const int y = (tile / k.tiles_x) * kGT + (int)(threadIdx.x >> 4);
    float dx, dy, dz;
    pixel_ray(r, x, y, dx, dy, dz);
    float best = __builtin_inff();
    int hit = -1;
    const uint32_t beg = k.offset[tile], end = k.offset[tile + 1];
    for (uint32_t base = beg; base < end; base += kRayChunk) {
        __syncthreads();
        const uint32_t cnt = min((uint32_t)kRayChunk, end - base);
        if (threadIdx.x < cnt) {
            const uint32_t t = k.bins[base + threadIdx.x];
            // masked: a mask word whose map is a texture of the moment (a stale index is no mask)
            const uint32_t mw = t < c.n_cut ? c.tri[t].x : kOpaque;
            const bool masked = mw != kOpaque && (mw >> 2) < r.n_tex;
            sid[threadIdx.x] = t | (masked ? kMaskedBit : 0u);
            sh[3 * threadIdx.x] = r.tri[(size_t)t * 4];
            sh[3 * threadIdx.x + 1] = r.tri[(size_t)t * 4 + 1];
            sh[3 * threadIdx.x + 2] = r.tri[(size_t)t * 4 + 2];
        }
        __syncthreads();
        for (uint32_t j = 0; j < cnt; ++j) {
            const float t = ray_tri(sh[3 * j], sh[3 * j + 1], sh[3 * j + 2], r.px, r.py, r.pz, dx, dy, dz);
            const uint32_t word = sid[j];
            const int id = (int)(word & ~kMaskedBit);
            if (t > 0.0f && (t < best || (t == best && id < hit))) {
                if (word & kMaskedBit) {   // the candidate would win now: is its point there?
                    float b1, b2, u, v;
                    ray_tri_bary(sh[3 * j], sh[3 * j + 1], sh[3 * j + 2], r.px, r.py, r.pz, dx, dy, dz, b1, b2);
                    const float4 a = r.uv[(size_t)id * 2], b = r.uv[(size_t)id * 2 + 1];
                    const float uv[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
                    tri_uv(uv, b1, b2, u, v);
                    const uint2 m = c.tri[id];
                    if (!covered(r.texels, r.tdesc, m.x, __uint_as_float(m.y), u, v)) continue;
                }
                best = t;
                hit = id;
            }
        }
    }
    if (x >= r.w || y >= r.h) return;
    if constexpr (SHADED) write_shaded(r, s, x, y, dx, dy, dz, best, hit);
    else write_gbuffer(r, x, y, dx, dy, dz, best, hit);
}

// grows *p to at least `bytes` (the ctx stream has drained: nothing reads the old block)
hipError_t grow(void** p, size_t* cap, size_t bytes) {
    if (*cap >= bytes) return hipSuccess;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) *cap = bytes;
    return e;
}

}  // namespace

void launch_cutout_setup(vct_ctx* c, const K1SetupArgs& a, const CutoutPass& cut) {
    hipLaunchKernelGGL(k1_tri_setup_cutout, dim3((a.n_tri + 255) / 256), dim3(256), 0, c->stream, a, cut.table, cut.tri);
}

void launch_cutout_candidates(vct_ctx* c, uint32_t blocks, bool packed, const void* geom, const void* fix,
                              const unsigned long long* offs, uint32_t n_tri, const unsigned long long* total,
                              const uint32_t* starts, const void* tuv) {
    Grid& g = c->grid;
    if (packed)
        hipLaunchKernelGGL(k1_candidates_cutout<true>, dim3(blocks), dim3(256), 0, c->stream, (const TriGeom*)geom,
                           (const TriFix*)fix, offs, n_tri, total, (int)g.n, g.accum, g.occ_bits, starts,
                           (const TriUV*)tuv, c->tex.texels, c->tex.desc);
    else
        hipLaunchKernelGGL(k1_candidates_cutout<false>, dim3(blocks), dim3(256), 0, c->stream, (const TriGeom*)geom,
                           (const TriFix*)fix, offs, n_tri, total, (int)g.n, g.accum, g.occ_bits, starts,
                           (const TriUV*)tuv, c->tex.texels, c->tex.desc);
}

const char* cutout_table_error(const vct_ctx* c, const vct_cutout* table, uint32_t n_mat) {
    if (!table) return nullptr;
    if (n_mat == 0) return "material_cutout with n_materials == 0";
    for (uint32_t i = 0; i < n_mat; ++i) {
        const vct_cutout& t = table[i];
        if (t.map < -1 || (t.map >= 0 && (uint32_t)t.map >= c->tex.n))
            return "material_cutout: map below -1 or not a texture of vct_set_textures";
        if (t.channel > 3) return "material_cutout: channel > 3";
        if (!(std::isfinite(t.cutoff) && t.cutoff > 0.0f && t.cutoff <= 1.0f))
            return "material_cutout: cutoff not finite or outside 0 < cutoff <= 1";
        if (t.reserved != 0) return "material_cutout: reserved != 0";
    }
    return nullptr;
}

uint32_t cutout_masked(const vct_cutout* table, uint32_t n_mat) {
    uint32_t n = 0;
    for (uint32_t i = 0; table && i < n_mat; ++i) n += table[i].map >= 0 ? 1u : 0u;
    return n;
}

hipError_t cutout_begin(vct_ctx* c, const vct_cutout* table, uint32_t n_mat, uint32_t n_tri, CutoutPass* pass) {
    Cutout& k = c->cut;
    k.live = false;
    hipError_t e;
    const size_t tri_bytes = (size_t)(n_tri ? n_tri : 1) * sizeof(uint2), tab_bytes = (size_t)n_mat * sizeof(vct_cutout);
    if (k.tri_cap < tri_bytes || k.table_cap < tab_bytes) {
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return e;
        if ((e = grow((void**)&k.tri, &k.tri_cap, tri_bytes)) != hipSuccess) return e;
        if ((e = grow((void**)&k.table, &k.table_cap, tab_bytes)) != hipSuccess) return e;
    }
    // (the caller waits for the ctx stream before it returns: the host table is free by then)
    if ((e = hipMemcpyAsync(k.table, table, tab_bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return e;
    pass->table = k.table;
    pass->tri = k.tri;
    return hipSuccess;
}

void cutout_commit(vct_ctx* c, const vct_cutout* table, uint32_t n_mat, uint32_t n_tri) {
    Cutout& k = c->cut;
    k.n_tri = n_tri;
    k.n_masked = cutout_masked(table, n_mat);
    k.epoch = c->grid_epoch;
    k.live = true;
}

void cutout_free(vct_ctx* c) {
    Cutout& k = c->cut;
    if (k.tri) (void)hipFree(k.tri);
    if (k.table) (void)hipFree(k.table);
    k = Cutout{};
}

}  // namespace vct

using namespace vct;

extern "C" vct_status vct_gbuffer_cutout_device(vct_ctx* c, const vct_camera* cam, uint32_t w, uint32_t h, float rough,
                                                float* pos4, float* nrm4, float* alb4, float* ks4, float* geo4,
                                                uint32_t* tri_id, float* bary2) {
    if (!c) return VCT_EINVAL;
    if (!cam || !pos4 || !nrm4 || !alb4) return lfail(c, VCT_EINVAL, "gbuffer_cutout: NULL camera or required plane");
    if (!ks4 && (geo4 || tri_id || bary2))
        return lfail(c, VCT_EINVAL, "gbuffer_cutout: geo4, tri_id and bary2 belong to the shaded records (ks4 is NULL)");
    if (const char* bad = gbuffer_input_error(cam, w, h)) return lfail(c, VCT_EINVAL, bad);
    if ((((uintptr_t)pos4 | (uintptr_t)nrm4 | (uintptr_t)alb4 | (uintptr_t)ks4 | (uintptr_t)geo4) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "gbuffer_cutout: float4 planes must be 16-byte aligned");
    if (((uintptr_t)tri_id & 3u) != 0 || ((uintptr_t)bary2 & 7u) != 0)
        return lfail(c, VCT_EINVAL, "gbuffer_cutout: tri_id must be 4-byte, bary2 8-byte aligned");
    if (!c->mesh.tri) return lfail(c, VCT_ESTATE, "gbuffer_cutout before voxelize");
    if (ks4 && !shading_live(c)) return lfail(c, VCT_ESTATE, "gbuffer_cutout: ks4 without a shading set (vct_set_shading)");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    BinK k;
    if ((e = gbuffer_bins(c, cam, w, h, rough, (float4*)pos4, (float4*)nrm4, (float4*)alb4, &k)) != hipSuccess)
        return lhip(c, e, "gbuffer_cutout: binning");
    CutK ck{nullptr, 0u};
    if (cutout_live(c) && c->cut.n_masked && k.r.uv) {
        ck.tri = c->cut.tri;
        ck.n_cut = c->cut.n_tri < c->mesh.n_tri ? c->cut.n_tri : c->mesh.n_tri;
    }
    const dim3 grid((uint32_t)(k.tiles_x * k.tiles_y));
    if (ks4) {
        const ShadeK s = shade_params(c, ks4, geo4, tri_id, bary2);
        hipLaunchKernelGGL(k_bin_raster_cutout<true>, grid, dim3(256), 0, c->stream, k, s, ck);
    } else {
        hipLaunchKernelGGL(k_bin_raster_cutout<false>, grid, dim3(256), 0, c->stream, k, ShadeK{}, ck);
    }
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "gbuffer_cutout");
    return VCT_OK;
}

extern "C" uint32_t vct_cutout_materials(const vct_ctx* c) { return c && cutout_live(c) ? c->cut.n_masked : 0u; }
