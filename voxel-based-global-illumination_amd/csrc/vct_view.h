// vct_view.h — the two device functions every unit that looks at a frame shares: the primary
// ray of a pixel (the G-buffer caster of vct_frame.hip, and the background rays of
// vct_fog.hip) and the present step's tone curve (every composite, and vct_fog_apply_device).
// One definition each, so the units cannot drift apart.  Internal to the including
// translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "vct_internal.h"

namespace vct {
namespace {

// The camera fields of a kernel record K: int w, h; float fx, fy, fz, ux, uy, uz, rx, ry, rz,
// tan_half, aspect (reference camera, r_voxelization.cpp:16-23: vertical FOV = zoom).
template <class K>
inline void camera_fields(K& k, const vct_camera* cam, uint32_t w, uint32_t h) {
    k.w = (int)w; k.h = (int)h;
    k.fx = cam->front[0]; k.fy = cam->front[1]; k.fz = cam->front[2];
    k.ux = cam->up[0]; k.uy = cam->up[1]; k.uz = cam->up[2];
    k.rx = cam->right[0]; k.ry = cam->right[1]; k.rz = cam->right[2];
    k.tan_half = tanf(cam->zoom_deg * 0.5f * 3.14159265358979f / 180.0f);
    k.aspect = (float)w / (float)h;
}

// pixel (x, y) -> unit ray direction (row 0 = top)
template <class K>
__device__ __forceinline__ void pixel_ray(const K& k, int x, int y, float& dx, float& dy, float& dz) {
    const float ndx = (2.0f * ((float)x + 0.5f) / (float)k.w - 1.0f) * k.tan_half * k.aspect;
    const float ndy = (1.0f - 2.0f * ((float)y + 0.5f) / (float)k.h) * k.tan_half;
    dx = k.fx + ndx * k.rx + ndy * k.ux;
    dy = k.fy + ndx * k.ry + ndy * k.uy;
    dz = k.fz + ndx * k.rz + ndy * k.uz;
    const float il = 1.0f / sqrtf(dot3(dx, dy, dz, dx, dy, dz));
    dx *= il; dy *= il; dz *= il;
}

// the present step: Reinhard and gamma 1/2.2 (tone01), then 8 bits, round half away (quant8)
__device__ __forceinline__ float tone01(float v) {
    v = v / (1.0f + v);
    return powf(v < 0.0f ? 0.0f : v, VCT_INV_GAMMA);
}
__device__ __forceinline__ uint32_t quant8(float v) {
    const int q = (int)lroundf(v * 255.0f);
    return (uint32_t)(q < 0 ? 0 : (q > 255 ? 255 : q));
}
__device__ __forceinline__ uint32_t to8(float v) { return quant8(tone01(v)); }

}  // namespace
}  // namespace vct
