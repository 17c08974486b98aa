// vct_shaded.h — what the shaded pass of vct_shading.hip and the cutout pass of vct_cutout.hip
// share: the shading set's kernel record, the presence bits of an attribute record, and the
// writer of a shaded texel (vct_spec.h "shading attributes").  One definition each, so the passes
// cannot drift apart.  Internal to the including translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include "vct_internal.h"
#include "vct_gbuffer.h"

namespace vct {
namespace {

constexpr uint32_t kShadeNormal = 1u, kShadeUv = 2u, kShadeTangent = 4u, kShadeBitangent = 8u;

struct ShadeK {
    const float4* rec;     // [n_set][9]
    const float4* mats;    // [n_mat][2]: (ks, roughness), (normal map, specular map, flags, 0) as bits
    uint32_t n_set, n_mat;
    float4* ks;
    float4* geo;           // NULL ok
    uint32_t* tri_id;      // NULL ok
    float2* bary;          // NULL ok
};

// the live set of the context (shading_live) and a call's output planes as a kernel record
inline ShadeK shade_params(const vct_ctx* c, float* ks4, float* geo4, uint32_t* tri_id, float* bary2) {
    ShadeK s;
    s.rec = c->shade.rec; s.mats = c->shade.mats;
    s.n_set = c->shade.n_tri < c->mesh.n_tri ? c->shade.n_tri : c->mesh.n_tri;
    s.n_mat = c->shade.n_mat;
    s.ks = (float4*)ks4; s.geo = (float4*)geo4; s.tri_id = tri_id; s.bary = (float2*)bary2;
    return s;
}

// a = fmaf(b2, a2 - a0, fmaf(b1, a1 - a0, a0)): tri_uv's form
__device__ __forceinline__ float lerp3(float a0, float a1, float a2, float b1, float b2) {
    return fmaf(b2, a2 - a0, fmaf(b1, a1 - a0, a0));
}

// v / sqrtf(dot3(v, v)) where the square is finite and > 0; false: no unit vector
__device__ __forceinline__ bool unit3(float& x, float& y, float& z) {
    const float sq = dot3(x, y, z, x, y, z);
    if (!(__builtin_isfinite(sq) && sq > 0.0f)) return false;
    const float l = sqrtf(sq);
    x /= l; y /= l; z /= l;
    return true;
}

// The texel of the nearest hit: write_gbuffer's (vct_gbuffer.h) operations for pos, the face
// normal and the albedo, then the shading attributes of the winner
__device__ __forceinline__ void write_shaded(const RayK& k, const ShadeK& s, int x, int y, float dx, float dy, float dz,
                                             float best, int hit) {
    const size_t p = (size_t)y * k.w + x;
    const float depth = best * dot3(dx, dy, dz, k.fx, k.fy, k.fz);
    if (hit < 0 || depth < k.near_p || depth > k.far_p) {
        const float4 z = make_float4(0, 0, 0, 0);
        k.pos[p] = z;
        k.nrm[p] = z;
        k.alb[p] = make_float4(0, 0, 0, k.rough);
        s.ks[p] = z;
        if (s.geo) s.geo[p] = z;
        if (s.tri_id) s.tri_id[p] = 0xFFFFFFFFu;
        if (s.bary) s.bary[p] = make_float2(0.0f, 0.0f);
        return;
    }
    const float4 v0 = k.tri[(size_t)hit * 4], e1 = k.tri[(size_t)hit * 4 + 1], e2 = k.tri[(size_t)hit * 4 + 2],
                 kd = k.tri[(size_t)hit * 4 + 3];
    float gx = e1.y * e2.z - e1.z * e2.y, gy = e1.z * e2.x - e1.x * e2.z, gz = e1.x * e2.y - e1.y * e2.x;
    const float nl = sqrtf(dot3(gx, gy, gz, gx, gy, gz));
    gx /= nl; gy /= nl; gz /= nl;
    const bool flipped = dot3(gx, gy, gz, dx, dy, dz) > 0.0f;
    if (flipped) { gx = -gx; gy = -gy; gz = -gz; }
    k.pos[p] = make_float4(k.px + dx * best, k.py + dy * best, k.pz + dz * best, 1.0f);
    float b1, b2;
    ray_tri_bary(v0, e1, e2, k.px, k.py, k.pz, dx, dy, dz, b1, b2);
    float ar = kd.x, ag = kd.y, ab = kd.z;
    const int tex = __float_as_int(kd.w);
    if (k.uv && tex >= 0 && (uint32_t)tex < k.n_tex) {   // albedo = Kd x T(uv of the hit), as write_gbuffer
        float u, v, tr, tg, tb;
        const float4 a = k.uv[(size_t)hit * 2], b = k.uv[(size_t)hit * 2 + 1];
        const float uv[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
        tri_uv(uv, b1, b2, u, v);
        tex_sample(k.texels, k.tdesc[tex], u, v, tr, tg, tb);
        ar = kd.x * tr; ag = kd.y * tg; ab = kd.z * tb;
    }
    // the flat record: a hit outside the set (a dynamic-layer triangle)
    float nx = gx, ny = gy, nz = gz, rough = k.rough, sr = 1.0f, sg = 1.0f, sb = 1.0f;
    if ((uint32_t)hit < s.n_set) {
        const float4* r = s.rec + 9 * (size_t)hit;
        const float4 q2 = r[2], q5 = r[5];
        const uint32_t mi = __float_as_uint(q2.w), present = __float_as_uint(q5.w);
        if (mi < s.n_mat) {
            const float4 m0 = s.mats[2 * (size_t)mi], m1 = s.mats[2 * (size_t)mi + 1];
            const int nmap = __float_as_int(m1.x), smap = __float_as_int(m1.y);
            const uint32_t flags = __float_as_uint(m1.z);
            const float4 q0 = r[0], q3 = r[3], q6 = r[6];
            // N0: the interpolated vertex normal, or Ng
            float n0x = gx, n0y = gy, n0z = gz;
            if (present & kShadeNormal) {
                float ix = lerp3(q0.x, q3.x, q6.x, b1, b2), iy = lerp3(q0.y, q3.y, q6.y, b1, b2),
                      iz = lerp3(q0.z, q3.z, q6.z, b1, b2);
                if (unit3(ix, iy, iz)) {
                    n0x = flipped ? -ix : ix; n0y = flipped ? -iy : iy; n0z = flipped ? -iz : iz;
                }
            }
            const bool has_uv = (present & kShadeUv) != 0;
            float u = 0.0f, v = 0.0f;
            if (has_uv) {
                const float4 q1 = r[1], q4 = r[4], q7 = r[7];
                u = lerp3(q0.w, q3.w, q6.w, b1, b2);
                v = lerp3(q1.w, q4.w, q7.w, b1, b2);
            }
            // N1: the tangent-space normal map over (T, B, N0), or N0
            float n1x = n0x, n1y = n0y, n1z = n0z;
            if (nmap >= 0 && (uint32_t)nmap < k.n_tex && has_uv && (present & kShadeTangent) && (present & kShadeBitangent)) {
                const float4 q1 = r[1], q4 = r[4], q7 = r[7], q8 = r[8];
                float cr, cg, cb;
                tex_sample(k.texels, k.tdesc[nmap], u, v, cr, cg, cb);
                const float mx = fmaf(2.0f, cr, -1.0f), mz = fmaf(2.0f, cb, -1.0f);
                float my = fmaf(2.0f, cg, -1.0f);
                if (flags & VCT_SHADING_FLIP_GREEN) my = -my;
                float tx = lerp3(q1.x, q4.x, q7.x, b1, b2), ty = lerp3(q1.y, q4.y, q7.y, b1, b2),
                      tz = lerp3(q1.z, q4.z, q7.z, b1, b2);
                float bx = lerp3(q2.x, q5.x, q8.x, b1, b2), by = lerp3(q2.y, q5.y, q8.y, b1, b2),
                      bz = lerp3(q2.z, q5.z, q8.z, b1, b2);
                if (flipped) { tx = -tx; ty = -ty; tz = -tz; bx = -bx; by = -by; bz = -bz; }
                float wx = (mx * tx + my * bx) + mz * n0x, wy = (mx * ty + my * by) + mz * n0y,
                      wz = (mx * tz + my * bz) + mz * n0z;
                if (unit3(wx, wy, wz)) { n1x = wx; n1y = wy; n1z = wz; }
            }
            // a shading normal never faces away from the viewer
            if (dot3(n1x, n1y, n1z, dx, dy, dz) < 0.0f) { nx = n1x; ny = n1y; nz = n1z; }
            rough = m0.w;
            sr = m0.x; sg = m0.y; sb = m0.z;
            if (smap >= 0 && (uint32_t)smap < k.n_tex && has_uv) {
                float tr, tg, tb;
                tex_sample(k.texels, k.tdesc[smap], u, v, tr, tg, tb);
                sr = m0.x * tr; sg = m0.y * tg; sb = m0.z * tb;
            }
        }
    }
    k.nrm[p] = make_float4(nx, ny, nz, 0.0f);
    k.alb[p] = make_float4(ar, ag, ab, rough);
    s.ks[p] = make_float4(sr, sg, sb, 1.0f);
    if (s.geo) s.geo[p] = make_float4(gx, gy, gz, 0.0f);
    if (s.tri_id) s.tri_id[p] = (uint32_t)hit;
    if (s.bary) s.bary[p] = make_float2(b1, b2);
}

}  // namespace
}  // namespace vct
