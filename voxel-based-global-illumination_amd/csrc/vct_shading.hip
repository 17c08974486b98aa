// vct_shading.hip — the shading G-buffer (include/vct_shading.h; vct_spec.h "shading
// attributes"):
//  * k_shade_setup: gathers the three vertices of every static triangle into one record of
//    nine float4 (Shading, vct_internal.h), so that every fetch of the pass is a 16-byte load;
//  * k_bin_raster_shaded: k_bin_raster's candidate loop over the bins of vct_frame.hip's
//    binning, unchanged (the same LDS staging, ties to the lower index), then once per pixel,
//    for the winner only, the attribute fetch, the two texture samples and the writes;
//  * k_spec_tint: out.rgb = spec.rgb * ks.rgb.
#include <cstring>
#include "vct_internal.h"
#include "vct_view.h"
#include "vct_gbuffer.h"
#include "vct_shaded.h"

namespace vct {
namespace {

struct SetupK {
    const char* verts;
    const uint32_t* idx;
    const uint32_t* mat;           // NULL: material 0
    uint32_t stride, n_verts, n_tri;
    uint32_t off_n, off_uv, off_t, off_b;   // VCT_SHADING_NO_ATTR: absent
    float4* rec;
};

__device__ __forceinline__ float3 attr3(const char* v, uint32_t off) {
    if (off == VCT_SHADING_NO_ATTR) return make_float3(0.0f, 0.0f, 0.0f);
    const float* p = (const float*)(v + off);
    return make_float3(p[0], p[1], p[2]);
}

__global__ void __launch_bounds__(256) k_shade_setup(SetupK k) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= k.n_tri) return;
    const uint32_t present = (k.off_n != VCT_SHADING_NO_ATTR ? kShadeNormal : 0u) | (k.off_uv != VCT_SHADING_NO_ATTR ? kShadeUv : 0u) |
                             (k.off_t != VCT_SHADING_NO_ATTR ? kShadeTangent : 0u) |
                             (k.off_b != VCT_SHADING_NO_ATTR ? kShadeBitangent : 0u);
    const uint32_t word[3] = {k.mat ? k.mat[t] : 0u, present, 0u};
    for (int j = 0; j < 3; ++j) {
        const uint32_t i = k.idx[3 * (size_t)t + j];
        float3 n = make_float3(0.0f, 0.0f, 0.0f), tg = n, bt = n;
        float u = 0.0f, v = 0.0f;
        if (i < k.n_verts) {   // (the host has checked every index; an all-zero vertex otherwise)
            const char* p = k.verts + (size_t)i * k.stride;
            n = attr3(p, k.off_n); tg = attr3(p, k.off_t); bt = attr3(p, k.off_b);
            if (k.off_uv != VCT_SHADING_NO_ATTR) { u = ((const float*)(p + k.off_uv))[0]; v = ((const float*)(p + k.off_uv))[1]; }
        }
        float4* r = k.rec + 9 * (size_t)t + 3 * j;
        r[0] = make_float4(n.x, n.y, n.z, u);
        r[1] = make_float4(tg.x, tg.y, tg.z, v);
        r[2] = make_float4(bt.x, bt.y, bt.z, __uint_as_float(word[j]));
    }
}

// (ShadeK, write_shaded and its helpers are vct_shaded.h's, shared with vct_cutout.hip)

// The texel's live state (two texture samples, three interpolated frames) would cost the loop one
// wave of occupancy (72 VGPRs: 7 waves per SIMD); held to k_bin_raster's 8 waves, the register
// allocator keeps it within 64 without a spill (DESIGN 10.14 has both kernels' figures)
__global__ void __launch_bounds__(256, 8) k_bin_raster_shaded(BinK k, ShadeK s) {
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
            sid[threadIdx.x] = t;
            sh[3 * threadIdx.x] = r.tri[(size_t)t * 4];
            sh[3 * threadIdx.x + 1] = r.tri[(size_t)t * 4 + 1];
            sh[3 * threadIdx.x + 2] = r.tri[(size_t)t * 4 + 2];
        }
        __syncthreads();
        for (uint32_t j = 0; j < cnt; ++j) {
            const float t = ray_tri(sh[3 * j], sh[3 * j + 1], sh[3 * j + 2], r.px, r.py, r.pz, dx, dy, dz);
            const int id = (int)sid[j];
            if (t > 0.0f && (t < best || (t == best && id < hit))) { best = t; hit = id; }
        }
    }
    if (x >= r.w || y >= r.h) return;
    write_shaded(r, s, x, y, dx, dy, dz, best, hit);
}

__global__ void __launch_bounds__(256) k_spec_tint(const float4* spec, const float4* ks, uint32_t n, float4* out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 s = spec[i], t = ks[i];
    out[i] = make_float4(s.x * t.x, s.y * t.y, s.z * t.z, s.w);
}

// a present attribute of `bytes` bytes at `off` in a vertex of `stride` bytes
bool attr_fits(uint32_t off, uint32_t bytes, uint32_t stride) {
    return off == VCT_SHADING_NO_ATTR || (off % 4 == 0 && (uint64_t)off + bytes <= stride);
}

// the material rule of vct_set_shading: nullptr, or what is wrong
const char* material_error(const vct_shading_material& m, uint32_t n_tex) {
    if (check_color(m.ks)) return "ks not finite, negative or above VCT_COLOR_LIMIT";
    if (!(m.roughness >= 0.0f && m.roughness <= 1.0f)) return "roughness not finite or outside [0, 1]";
    for (int32_t map : {m.normal_map, m.specular_map})
        if (map < -1 || (map >= 0 && (uint32_t)map >= n_tex)) return "map index below -1 or beyond the texture set";
    if (m.flags & ~VCT_SHADING_FLIP_GREEN) return "unknown flag bits";
    if (m.reserved != 0) return "reserved != 0";
    return nullptr;
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

void shading_free(vct_ctx* c) {
    Shading& s = c->shade;
    if (s.rec) (void)hipFree(s.rec);
    if (s.mats) (void)hipFree(s.mats);
    s = Shading{};
}

}  // namespace vct

using namespace vct;

extern "C" vct_status vct_set_shading(vct_ctx* c, const vct_shading_desc* d) {
    if (!c) return VCT_EINVAL;
    hipError_t e;
    if (!d) {   // clear the set (the pass that may still read it runs on the ctx stream)
        if ((e = hipSetDevice(c->device)) != hipSuccess) return lhip(c, e, "hipSetDevice");
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return lhip(c, e, "set_shading: stream synchronize");
        shading_free(c);
        return VCT_OK;
    }
    if (!c->grid.voxelized || !c->mesh.tri) return lfail(c, VCT_ESTATE, "set_shading before voxelize");
    if (!d->verts || !d->idx || !d->materials || d->n_materials == 0)
        return lfail(c, VCT_EINVAL, "set_shading: NULL verts, idx or materials, or n_materials == 0");
    const uint32_t n_static = static_triangles(c);
    if (d->n_idx % 3 != 0 || d->n_idx / 3 != n_static)
        return lfail(c, VCT_EINVAL, "set_shading: n_idx = " + std::to_string(d->n_idx) + ", the static voxelization has " +
                                        std::to_string(n_static) + " triangles");
    if (!attr_fits(d->normal_offset, 12, d->vertex_stride) || !attr_fits(d->uv_offset, 8, d->vertex_stride) ||
        !attr_fits(d->tangent_offset, 12, d->vertex_stride) || !attr_fits(d->bitangent_offset, 12, d->vertex_stride))
        return lfail(c, VCT_EINVAL, "set_shading: a present offset must be a multiple of 4 and end within vertex_stride");
    for (uint32_t i = 0; i < d->n_idx; ++i)
        if (d->idx[i] >= d->n_verts) return lfail(c, VCT_EINVAL, "set_shading: vertex index out of range");
    for (uint32_t t = 0; d->tri_material && t < n_static; ++t)
        if (d->tri_material[t] >= d->n_materials)
            return lfail(c, VCT_EINVAL, "set_shading: tri_material[" + std::to_string(t) + "] >= n_materials");
    for (uint32_t m = 0; m < d->n_materials; ++m)
        if (const char* bad = material_error(d->materials[m], c->tex.n))
            return lfail(c, VCT_EINVAL, "set_shading: material " + std::to_string(m) + ": " + bad);
    if ((e = hipSetDevice(c->device)) != hipSuccess) return lhip(c, e, "hipSetDevice");
    // from here on the previous set is gone
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return lhip(c, e, "set_shading: stream synchronize");
    Shading& s = c->shade;
    s.live = false;
    const size_t rec_bytes = (size_t)(n_static ? n_static : 1) * 9 * sizeof(float4);
    const size_t mat_bytes = (size_t)d->n_materials * sizeof(vct_shading_material);
    if ((e = grow((void**)&s.rec, &s.rec_cap, rec_bytes)) != hipSuccess) return lhip(c, e, "hipMalloc shading records");
    if ((e = grow((void**)&s.mats, &s.mat_cap, mat_bytes)) != hipSuccess) return lhip(c, e, "hipMalloc shading materials");
    MeshStage ms;
    const size_t vbytes = (size_t)d->vertex_stride * d->n_verts;
    if (n_static) {
        const vct_status st = stage_mesh(c, ms, d->verts, vbytes, d->idx, d->n_idx, d->tri_material, nullptr, "", nullptr, 0);
        if (st != VCT_OK) return st;
        SetupK k;
        k.verts = (const char*)ms.verts.p; k.idx = (const uint32_t*)ms.idx.p; k.mat = (const uint32_t*)ms.mat.p;
        k.stride = d->vertex_stride; k.n_verts = d->n_verts; k.n_tri = n_static;
        k.off_n = d->normal_offset; k.off_uv = d->uv_offset; k.off_t = d->tangent_offset; k.off_b = d->bitangent_offset;
        k.rec = s.rec;
        hipLaunchKernelGGL(k_shade_setup, dim3((n_static + 255) / 256), dim3(256), 0, c->stream, k);
        if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "set_shading: setup");
    }
    if ((e = hipMemcpyAsync(s.mats, d->materials, mat_bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess)
        return lhip(c, e, "set_shading: upload materials");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return lhip(c, e, "set_shading: sync");
    s.n_tri = n_static;
    s.n_mat = d->n_materials;
    s.epoch = c->grid_epoch;
    s.live = true;
    return VCT_OK;
}

extern "C" vct_status vct_gbuffer_shaded_device(vct_ctx* c, const vct_camera* cam, uint32_t w, uint32_t h, float rough,
                                                float* pos4, float* nrm4, float* alb4, float* ks4, float* geo4,
                                                uint32_t* tri_id, float* bary2) {
    if (!c) return VCT_EINVAL;
    if (!cam || !pos4 || !nrm4 || !alb4 || !ks4) return lfail(c, VCT_EINVAL, "gbuffer_shaded: NULL camera or required plane");
    if (const char* bad = gbuffer_input_error(cam, w, h)) return lfail(c, VCT_EINVAL, bad);
    if ((((uintptr_t)pos4 | (uintptr_t)nrm4 | (uintptr_t)alb4 | (uintptr_t)ks4 | (uintptr_t)geo4) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "gbuffer_shaded: float4 planes must be 16-byte aligned");
    if (((uintptr_t)tri_id & 3u) != 0 || ((uintptr_t)bary2 & 7u) != 0)
        return lfail(c, VCT_EINVAL, "gbuffer_shaded: tri_id must be 4-byte, bary2 8-byte aligned");
    if (!c->mesh.tri) return lfail(c, VCT_ESTATE, "gbuffer_shaded before voxelize");
    if (!shading_live(c)) return lfail(c, VCT_ESTATE, "gbuffer_shaded without a shading set (vct_set_shading)");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    BinK k;
    if ((e = gbuffer_bins(c, cam, w, h, rough, (float4*)pos4, (float4*)nrm4, (float4*)alb4, &k)) != hipSuccess)
        return lhip(c, e, "gbuffer_shaded: binning");
    const ShadeK s = shade_params(c, ks4, geo4, tri_id, bary2);
    hipLaunchKernelGGL(k_bin_raster_shaded, dim3((uint32_t)(k.tiles_x * k.tiles_y)), dim3(256), 0, c->stream, k, s);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "gbuffer_shaded");
    return VCT_OK;
}

extern "C" vct_status vct_specular_tint_device(vct_ctx* c, const float* spec4, const float* ks4, uint32_t w, uint32_t h,
                                               float* out4) {
    if (!c) return VCT_EINVAL;
    if (!spec4 || !ks4 || !out4) return lfail(c, VCT_EINVAL, "specular_tint: NULL plane");
    if ((((uintptr_t)spec4 | (uintptr_t)ks4 | (uintptr_t)out4) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "specular_tint: planes must be 16-byte aligned");
    const uint64_t px = (uint64_t)w * h;
    if (px == 0 || px > 0x7fffffffull) return lfail(c, VCT_EINVAL, "specular_tint: w * h outside 1..2^31 - 1");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    hipLaunchKernelGGL(k_spec_tint, dim3((uint32_t)((px + 255) / 256)), dim3(256), 0, c->stream, (const float4*)spec4,
                       (const float4*)ks4, (uint32_t)px, (float4*)out4);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "specular_tint");
    return VCT_OK;
}
