// vct_light_terms.h — what the translation units that evaluate a light list share
// (vct_lights.hip: K2 and the composite; vct_shadow.hip: shadow cones and their composite):
// a light with the spec's per-light constants, the per-receiver terms, the plain shadow
// walk, the host-side validation of a list, and the present step.  Everything is internal
// to the including translation unit (vct_spec.h "local lights" has the arithmetic).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "vct_internal.h"
#include "vct_view.h"

namespace vct {
namespace {

static_assert(sizeof(vct_light) == 60, "vct_light is 15 dwords (include/vct_lights.h)");

// a light with the per-light constants of the spec (13 dwords)
struct DLight {
    uint32_t type;
    float px, py, pz;        // pL: the position in voxel units (point, spot)
    float ax, ay, az;        // directional: l; spot: a = -axis
    float cr, cg, cb;
    float inv_rr;            // 1 / (range in voxels)^2
    float cos_outer, inv_span;
};
struct LightSet {
    DLight l[VCT_MAX_LIGHTS];
};

// The spec's per-receiver, per-light terms; false: the light is skipped.
__device__ __forceinline__ bool light_terms(const DLight& L, float h2, float qx, float qy, float qz, float nx, float ny,
                                            float nz, float& lx, float& ly, float& lz, float& f, float& ndl,
                                            float& t_lim) {
    if (L.type == VCT_LIGHT_DIRECTIONAL) {
        lx = L.ax; ly = L.ay; lz = L.az;
        f = 1.0f;
        t_lim = __builtin_inff();
    } else {
        const float dx = L.px - qx, dy = L.py - qy, dz = L.pz - qz;
        const float r2 = dot3(dx, dy, dz, dx, dy, dz);
        if (!(r2 > 0.0f)) return false;
        const float r = sqrtf(r2);
        lx = dx / r; ly = dy / r; lz = dz / r;
        t_lim = r;
        const float u = r2 * L.inv_rr;
        const float w = fmaxf(1.0f - u, 0.0f);
        f = (w * w) / (1.0f + r2 * h2);
        if (L.type == VCT_LIGHT_SPOT) {
            const float cd = dot3(lx, ly, lz, L.ax, L.ay, L.az);
            const float s = fminf(fmaxf((cd - L.cos_outer) * L.inv_span, 0.0f), 1.0f);
            f = f * (s * s);
        }
    }
    ndl = dot3(nx, ny, nz, lx, ly, lz);
    return ndl > 0.0f && f > 0.0f;
}

// The spec's V, plainly: dda_visibility (vct_device.h) with the entry parameter t_e of the
// current cell and the end t_e >= t_lim.  K2 input rule: an axis whose td is not finite does
// not move (s_a = 0, tm_a = +inf), so no t is ever NaN.
__device__ __forceinline__ float dda_lim(const unsigned long long* __restrict__ bits, int N, float qx, float qy,
                                         float qz, float lx, float ly, float lz, float t_lim) {
    int vx = (int)floorf(qx), vy = (int)floorf(qy), vz = (int)floorf(qz);
    if (vx < 0 || vy < 0 || vz < 0 || vx >= N || vy >= N || vz >= N) return 1.0f;
    int sx = lx > 0.0f ? 1 : (lx < 0.0f ? -1 : 0);
    int sy = ly > 0.0f ? 1 : (ly < 0.0f ? -1 : 0);
    int sz = lz > 0.0f ? 1 : (lz < 0.0f ? -1 : 0);
    const float inf = __builtin_inff();
    const float tdx = sx ? 1.0f / fabsf(lx) : inf;
    const float tdy = sy ? 1.0f / fabsf(ly) : inf;
    const float tdz = sz ? 1.0f / fabsf(lz) : inf;
    if (tdx == inf) sx = 0;
    if (tdy == inf) sy = 0;
    if (tdz == inf) sz = 0;
    float tmx = sx > 0 ? ((float)(vx + 1) - qx) * tdx : (sx < 0 ? (qx - (float)vx) * tdx : inf);
    float tmy = sy > 0 ? ((float)(vy + 1) - qy) * tdy : (sy < 0 ? (qy - (float)vy) * tdy : inf);
    float tmz = sz > 0 ? ((float)(vz + 1) - qz) * tdz : (sz < 0 ? (qz - (float)vz) * tdz : inf);
    float te = 0.0f;
    for (;;) {
        if (te >= t_lim) return 1.0f;
        if (occ_at(bits, N, vx, vy, vz)) return 0.0f;
        if (tmx <= tmy && tmx <= tmz) {
            te = tmx; vx += sx; if (vx < 0 || vx >= N) return 1.0f; tmx = tmx + tdx;
        } else if (tmy <= tmz) {
            te = tmy; vy += sy; if (vy < 0 || vy >= N) return 1.0f; tmy = tmy + tdy;
        } else {
            te = tmz; vz += sz; if (vz < 0 || vz >= N) return 1.0f; tmz = tmz + tdz;
        }
    }
}

// the present step's tone curve, to8, is vct_view.h's

// ---- host side --------------------------------------------------------------------------
bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// vct_light -> DLight by the spec's host arithmetic; nullptr, or what is wrong with the light
const char* prepare_light(const Grid& g, const vct_light& in, DLight& out) {
    if (in.type > VCT_LIGHT_SPOT) return "unknown light type";
    if (in.reserved[0] || in.reserved[1]) return "nonzero reserved words";
    if (!finite3(in.position) || !finite3(in.direction) || !finite3(in.color) || !std::isfinite(in.range) ||
        !std::isfinite(in.cos_inner) || !std::isfinite(in.cos_outer))
        return "non-finite field";
    if (const char* bad = check_color(in.color)) return bad;   // K2 input rule, colour (vct_internal.h)
    out = DLight{};
    out.type = in.type;
    out.cr = in.color[0]; out.cg = in.color[1]; out.cb = in.color[2];
    float ux = 0.0f, uy = 0.0f, uz = 0.0f;
    if (in.type != VCT_LIGHT_POINT) {
        const float dx = in.direction[0], dy = in.direction[1], dz = in.direction[2];
        // K2 input rule, direction: len in float32 finite and > 0 (a squared length that
        // underflows to 0 or overflows to +inf is refused)
        const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
        if (!(len > 0.0f) || !std::isfinite(len)) return "zero or non-finite light direction";
        ux = dx / len; uy = dy / len; uz = dz / len;
    }
    if (in.type == VCT_LIGHT_DIRECTIONAL) {
        out.ax = ux; out.ay = uy; out.az = uz;
        return nullptr;
    }
    if (!(in.range > 0.0f)) return "range <= 0";
    out.px = (in.position[0] - g.g0[0]) * g.inv_h;
    out.py = (in.position[1] - g.g0[1]) * g.inv_h;
    out.pz = (in.position[2] - g.g0[2]) * g.inv_h;
    const float rv = in.range * g.inv_h;
    out.inv_rr = 1.0f / (rv * rv);
    if (in.type == VCT_LIGHT_SPOT) {
        if (!(1.0f >= in.cos_inner && in.cos_inner > in.cos_outer && in.cos_outer >= 0.0f))
            return "spot cosines must satisfy 1 >= cos_inner > cos_outer >= 0";
        out.ax = -ux; out.ay = -uy; out.az = -uz;
        out.cos_outer = in.cos_outer;
        out.inv_span = 1.0f / (in.cos_inner - in.cos_outer);
    }
    return nullptr;
}

float grid_h2(const Grid& g) {
    const float hh = g.extent / (float)g.n;
    return hh * hh;
}

vct_status prepare_list(vct_ctx* c, const char* what, const vct_light* lights, uint32_t n, DLight* out) {
    if (n > VCT_MAX_LIGHTS) return lfail(c, VCT_EINVAL, std::string(what) + ": more than VCT_MAX_LIGHTS lights");
    if (n && !lights) return lfail(c, VCT_EINVAL, std::string(what) + ": NULL lights");
    for (uint32_t i = 0; i < n; ++i)
        if (const char* bad = prepare_light(c->grid, lights[i], out[i]))
            return lfail(c, VCT_EINVAL, std::string(what) + ": light " + std::to_string(i) + ": " + bad);
    return VCT_OK;
}

}  // namespace
}  // namespace vct
