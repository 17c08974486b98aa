// vct_gbuffer.h — what the G-buffer passes of vct_frame.hip, the shaded pass of
// vct_shading.hip and the cutout pass of vct_cutout.hip share: the kernel records, the
// Moller-Trumbore test and its barycentrics, the flat texel writer.  One definition each, so
// the passes cannot drift apart.  Internal to the including translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include "vct_internal.h"

namespace vct {

// ---- G-buffer ray caster (input producer for synthetic scenes) -----------
struct RayK {
    const float4* tri;  // [n][4]: v0, e1, e2, (kd, diffuse map as int bits)
    const float4* uv;   // [n][2] TexCoords of textured triangles (NULL: untextured voxelization)
    const uint32_t* texels;   // diffuse maps (vct_set_textures)
    const TexDesc* tdesc;
    uint32_t n_tex;
    uint32_t n_tri;
    int w, h;
    float px, py, pz;
    float fx, fy, fz, ux, uy, uz, rx, ry, rz;
    float tan_half, aspect, near_p, far_p, rough;
    float4* pos;
    float4* nrm;
    float4* alb;
};

constexpr int kRayChunk = 256;
constexpr int kGT = 16;   // pixels per side of a bin tile

struct BinK {
    RayK r;
    int tiles_x, tiles_y;
    float sxs, sys;                // pixel scale: X = w/2 + (cx/cz) sxs, Y = h/2 - (cy/cz) sys
    float t_near;                  // 2 kZc max|D|: a hit with cz < kZc has a ray parameter below half of this
    float pad;                     // 2^-20 s M^2: pixels of float32 slack per unit of a triangle's conditioning
    int4* rect;                    // per triangle tile rectangle (x0 > x1: culled)
    uint32_t* count;               // per tile: triangles, then the fill cursor
    uint32_t* offset;              // per tile: exclusive prefix of count; [n_tiles] = total
    uint32_t* bins;                // triangle indices grouped by tile
};

// The binned pass up to its last launch (vct_frame.hip): the bins of the frame, queued on the
// ctx stream (one 4-byte read back); *k is ready for a raster kernel over k->tiles_x *
// k->tiles_y workgroups
hipError_t gbuffer_bins(vct_ctx* c, const vct_camera* cam, uint32_t w, uint32_t h, float rough, float4* pos,
                        float4* nrm, float4* alb, BinK* k);

namespace {

// Moller-Trumbore: ray parameter t of the hit, or -1 (no hit / parallel)
__device__ __forceinline__ float ray_tri(float4 v0, float4 e1, float4 e2, float px, float py, float pz, float dx,
                                         float dy, float dz) {
    const float pvx = dy * e2.z - dz * e2.y, pvy = dz * e2.x - dx * e2.z, pvz = dx * e2.y - dy * e2.x;
    const float det = dot3(e1.x, e1.y, e1.z, pvx, pvy, pvz);
    if (fabsf(det) < 1e-12f) return -1.0f;
    const float inv = 1.0f / det;
    const float tx = px - v0.x, ty = py - v0.y, tz = pz - v0.z;
    const float u = dot3(tx, ty, tz, pvx, pvy, pvz) * inv;
    if (u < 0.0f || u > 1.0f) return -1.0f;
    const float qx = ty * e1.z - tz * e1.y, qy = tz * e1.x - tx * e1.z, qz = tx * e1.y - ty * e1.x;
    const float v = dot3(dx, dy, dz, qx, qy, qz) * inv;
    if (v < 0.0f || u + v > 1.0f) return -1.0f;
    return dot3(e2.x, e2.y, e2.z, qx, qy, qz) * inv;
}

// Moller-Trumbore barycentrics (u, v) of a ray known to hit the triangle (ray_tri's operations)
__device__ __forceinline__ void ray_tri_bary(float4 v0, float4 e1, float4 e2, float px, float py, float pz, float dx,
                                             float dy, float dz, float& u, float& v) {
    const float pvx = dy * e2.z - dz * e2.y, pvy = dz * e2.x - dx * e2.z, pvz = dx * e2.y - dy * e2.x;
    const float det = dot3(e1.x, e1.y, e1.z, pvx, pvy, pvz);
    const float inv = 1.0f / det;
    const float tx = px - v0.x, ty = py - v0.y, tz = pz - v0.z;
    u = dot3(tx, ty, tz, pvx, pvy, pvz) * inv;
    const float qx = ty * e1.z - tz * e1.y, qy = tz * e1.x - tx * e1.z, qz = tx * e1.y - ty * e1.x;
    v = dot3(dx, dy, dz, qx, qy, qz) * inv;
}

// G-buffer texel of the nearest hit (shared by the brute-force, the binned and the cutout pass)
__device__ __forceinline__ void write_gbuffer(const RayK& k, int x, int y, float dx, float dy, float dz, float best,
                                              int hit) {
    const size_t p = (size_t)y * k.w + x;
    const float depth = best * dot3(dx, dy, dz, k.fx, k.fy, k.fz);
    if (hit < 0 || depth < k.near_p || depth > k.far_p) {
        k.pos[p] = make_float4(0, 0, 0, 0);
        k.nrm[p] = make_float4(0, 0, 0, 0);
        k.alb[p] = make_float4(0, 0, 0, k.rough);
        return;
    }
    const float4 e1 = k.tri[(size_t)hit * 4 + 1], e2 = k.tri[(size_t)hit * 4 + 2], kd = k.tri[(size_t)hit * 4 + 3];
    float nx = e1.y * e2.z - e1.z * e2.y, ny = e1.z * e2.x - e1.x * e2.z, nz = e1.x * e2.y - e1.y * e2.x;
    const float nl = sqrtf(dot3(nx, ny, nz, nx, ny, nz));
    nx /= nl; ny /= nl; nz /= nl;
    if (dot3(nx, ny, nz, dx, dy, dz) > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    k.pos[p] = make_float4(k.px + dx * best, k.py + dy * best, k.pz + dz * best, 1.0f);
    k.nrm[p] = make_float4(nx, ny, nz, 0.0f);
    float ar = kd.x, ag = kd.y, ab = kd.z;
    const int tex = __float_as_int(kd.w);
    if (k.uv && tex >= 0 && (uint32_t)tex < k.n_tex) {   // albedo = Kd x T(uv of the hit)
        float b1, b2, u, v, tr, tg, tb;
        ray_tri_bary(k.tri[(size_t)hit * 4], e1, e2, k.px, k.py, k.pz, dx, dy, dz, b1, b2);
        const float4 a = k.uv[(size_t)hit * 2], b = k.uv[(size_t)hit * 2 + 1];
        const float uv[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
        tri_uv(uv, b1, b2, u, v);
        tex_sample(k.texels, k.tdesc[tex], u, v, tr, tg, tb);
        ar = kd.x * tr; ag = kd.y * tg; ab = kd.z * tb;
    }
    k.alb[p] = make_float4(ar, ag, ab, k.rough);
}

}  // namespace
}  // namespace vct
