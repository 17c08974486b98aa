// vct_sky_march.h — the three kernels behind the four sky calls, with their launchers and the
// bodies of the entry points, shared by the two families that differ only in the colour of a
// direction: vct_sky.hip (the three-colour gradient Sky(d)) and vct_env.hip (the octahedral map
// Env(d, tau)).  Everything is templated on that colour source Src: a small record passed by
// value inside the kernel's argument record, with one device function
//     void color(float dx, float dy, float dz, float tau, float& r, float& g, float& b) const;
// (the gradient ignores tau).  Device code is internal to the including translation unit, as
// vct_alpha_march.h's is.
//
//   ksky_march   the work shape of ks_march (vct_shadow.hip): one wave per 8x8 block, one lane
//                per record.  The cone loop is wave-uniform and in set order, so every
//                receiver's fmaf chain is its lane's own, in the spec's order, without an
//                atomic.  Each cone is vct_alpha_march.h's lockstep cone<> with t_lim = +inf.
//                The directions (K4's tangent frame of the lane's normal) are per lane, so the
//                faces and d^2 are per lane, as for ks_march's point lights.  The set's aperture
//                is wave-uniform, so a map's level pair is too; its taps are per lane.
//   ksky_spec    the same work shape, one lane per pixel.  The cone is K4's specular cone
//                reduced to its alpha channel; its aperture is the pixel's roughness, so it is
//                vct_alpha_march.h's per-lane cone_lane<>.  The colour is looked up at the
//                pixel's own aperture.
//   ksky_bg      a streaming kernel: one float4 load of pos4 per pixel, stores at background
//                pixels only, compiled once per set of outputs.  The colour at aperture 0.
//
// Every record is one lane's own, so the only atomic is the wave-summed step counter.
// Addresses: vct_alpha_march.h says how the marches' stay in range; a non-finite position,
// normal or direction fails the inside test, so such a pixel ends its cones before the first
// sample.  A source's own addresses are the source's to bound (vct_env.hip env_color).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstring>
#include <string>
#include "vct_internal.h"
#include "vct_light_terms.h"
#include "vct_alpha_march.h"
#include "vct_view.h"

namespace vct {
namespace {

template <class Src>
struct SkyMarchK {
    const float4* pos;
    const float4* nrm;
    const StepRow* tab;          // the diffuse aperture's step table, kShadowRows rows
    float4* sky;                 // [h][w]
    float4* diff;                // [h][w] or null: diffuse.rgb += sky.rgb
    unsigned long long* steps_total;
    AlphaRange lvl[kMaxLevels + 1];
    int n, L, lgn, aniso;
    int w, h, tiles_x, nd;
    float g0x, g0y, g0z, inv_h, tmax;
    float tau_set;               // the cone set's aperture
    Src s;
};

template <class Src>
struct SkySpecK {
    const float4* pos;
    const float4* nrm;
    const float4* alb;
    float4* out;                 // [h][w] (S.rgb, T)
    float4* spec;                // [h][w] or null: spec.rgb += S.rgb
    unsigned long long* steps_total;
    AlphaRange lvl[kMaxLevels + 1];
    int n, L, lgn, aniso;
    int w, h, tiles_x, march;    // march = 0: a context without a specular cone
    float g0x, g0y, g0z, inv_h, tmax;
    float ex, ey, ez;
    Src s;
};

template <class Src>
struct SkyBgK {
    const float4* pos;
    float4* lin;
    uint32_t* rgba8;
    uint32_t npx;
    int w, h;
    float fx, fy, fz, ux, uy, uz, rx, ry, rz, tan_half, aspect;   // vct_view.h camera_fields
    Src s;
};

#define VCT_SKY_ROW(cn, ct, cb, w) {cn, ct, cb, w},
__device__ const float kSkyCones1[1][4] = {VCT_CONES1(VCT_SKY_ROW)};
__device__ const float kSkyCones9[9][4] = {VCT_CONES9(VCT_SKY_ROW)};
__device__ const float kSkyCones16[16][4] = {VCT_CONES16(VCT_SKY_ROW)};
#undef VCT_SKY_ROW

// K4's tangent frame of a normal (A.5; Duff et al. 2017), the operations in K4's order
struct Frame {
    float Tx, Ty, Tz, Bx, By, Bz;
};
__device__ __forceinline__ Frame tangent_frame(float nx, float ny, float nz) {
    const float sgn = copysignf(1.0f, nz);
    const float ka = -1.0f / (sgn + nz);
    const float kb = (nx * ny) * ka;
    return Frame{1.0f + ((sgn * nx) * nx) * ka, sgn * kb, -(sgn * nx), kb, sgn + (ny * ny) * ka, -ny};
}

// A.6's specular cone, the operations in K4's order: the eye direction at P mirrored about the
// normal, and the roughness clamped to the apertures the march takes
__device__ __forceinline__ void specular_cone(float ex, float ey, float ez, const float4& P, float nx, float ny, float nz,
                                              float rough, float& dx, float& dy, float& dz, float& tau) {
    float vx = ex - P.x, vy = ey - P.y, vz = ez - P.z;
    const float vl = sqrtf(dot3(vx, vy, vz, vx, vy, vz));
    vx = vx / vl; vy = vy / vl; vz = vz / vl;
    const float ndv = dot3(nx, ny, nz, vx, vy, vz);
    const float k2 = 2.0f * ndv;
    dx = k2 * nx - vx; dy = k2 * ny - vy; dz = k2 * nz - vz;
    tau = fminf(fmaxf(rough, VCT_SPEC_TAU_MIN), VCT_SPEC_TAU_MAX);
}

template <bool O32, class Src>
__global__ void __launch_bounds__(64) ksky_march(const SkyMarchK<Src> k) {
    const int lane = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / k.tiles_x, tx = (int)blockIdx.x - ty * k.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const bool inframe = x < k.w && y < k.h;
    const size_t i = inframe ? (size_t)y * (size_t)k.w + (size_t)x : 0u;
    const float4 P = k.pos[i], N = k.nrm[i];
    const bool valid = inframe && P.w != 0.0f;
    if (__builtin_amdgcn_ballot_w64(valid) == 0ull) {          // a block of background
        if (inframe) k.sky[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float ox = (P.x - k.g0x) * k.inv_h + N.x, oy = (P.y - k.g0y) * k.inv_h + N.y,
                oz = (P.z - k.g0z) * k.inv_h + N.z;
    const float nx = N.x, ny = N.y, nz = N.z;
    const Frame f = tangent_frame(nx, ny, nz);
    const float(*cones)[4] = k.nd == 16 ? kSkyCones16 : (k.nd == 9 ? kSkyCones9 : kSkyCones1);
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, vis = 0.0f;
    uint32_t steps = 0;
    for (int c = 0; c < k.nd; ++c) {
        const float cn = cones[c][0], ct = cones[c][1], cb = cones[c][2], wk = cones[c][3];
        const float dx = (cn * nx + ct * f.Tx) + cb * f.Bx;
        const float dy = (cn * ny + ct * f.Ty) + cb * f.By;
        const float dz = (cn * nz + ct * f.Tz) + cb * f.Bz;
        const float a = cone<O32>(k, k.tab, valid, ox, oy, oz, dx, dy, dz, __builtin_inff(), steps);
        const float T = fmaxf(1.0f - a / VCT_ALPHA_STOP, 0.0f);
        float sr, sg, sb;
        k.s.color(dx, dy, dz, k.tau_set, sr, sg, sb);
        const float wt = wk * T;
        ar = fmaf(wt, sr, ar);
        ag = fmaf(wt, sg, ag);
        ab = fmaf(wt, sb, ab);
        vis = fmaf(wk, T, vis);
    }
    if (inframe) {
        k.sky[i] = valid ? make_float4(ar, ag, ab, vis) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k.diff && valid) {
            float4 D = k.diff[i];
            D.x = D.x + ar;
            D.y = D.y + ag;
            D.z = D.z + ab;
            k.diff[i] = D;
        }
    }
    if (k.steps_total) {
        const uint32_t ws = wave_sum_u32(steps);
        if (lane == 0 && ws) atomicAdd(k.steps_total, (unsigned long long)ws);
    }
}

template <bool O32, class Src>
__global__ void __launch_bounds__(64) ksky_spec(const SkySpecK<Src> k) {
    const int lane = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / k.tiles_x, tx = (int)blockIdx.x - ty * k.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const bool inframe = x < k.w && y < k.h;
    const size_t i = inframe ? (size_t)y * (size_t)k.w + (size_t)x : 0u;
    const float4 P = k.pos[i];
    const bool valid = inframe && P.w != 0.0f && k.march != 0;
    if (__builtin_amdgcn_ballot_w64(valid) == 0ull) {          // a block of background
        if (inframe) k.out[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 N = k.nrm[i];
    float rough = 0.1f;
    if (valid) rough = k.alb[i].w;
    const float nx = N.x, ny = N.y, nz = N.z;
    const float ox = (P.x - k.g0x) * k.inv_h + nx, oy = (P.y - k.g0y) * k.inv_h + ny,
                oz = (P.z - k.g0z) * k.inv_h + nz;
    float dx, dy, dz, tau;
    specular_cone(k.ex, k.ey, k.ez, P, nx, ny, nz, rough, dx, dy, dz, tau);
    uint32_t steps = 0;
    const float a = cone_lane<O32>(k, valid, ox, oy, oz, dx, dy, dz, tau, steps);
    if (inframe) {
        const float T = fmaxf(1.0f - a / VCT_ALPHA_STOP, 0.0f);
        float sr, sg, sb;
        k.s.color(dx, dy, dz, tau, sr, sg, sb);
        sr = T * sr; sg = T * sg; sb = T * sb;
        k.out[i] = valid ? make_float4(sr, sg, sb, T) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k.spec && valid) {
            float4 S = k.spec[i];
            S.x = S.x + sr;
            S.y = S.y + sg;
            S.z = S.z + sb;
            k.spec[i] = S;
        }
    }
    if (k.steps_total) {
        const uint32_t ws = wave_sum_u32(steps);
        if (lane == 0 && ws) atomicAdd(k.steps_total, (unsigned long long)ws);
    }
}

template <bool LIN, bool RGBA, class Src>
__global__ void __launch_bounds__(256) ksky_bg(const SkyBgK<Src> k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k.npx) return;
    const float4 P = k.pos[i];
    if (P.w != 0.0f) return;
    const int y = (int)(i / (uint32_t)k.w), x = (int)(i - (uint32_t)y * (uint32_t)k.w);
    float dx, dy, dz, r, g, b;
    pixel_ray(k, x, y, dx, dy, dz);
    k.s.color(dx, dy, dz, 0.0f, r, g, b);
    if constexpr (LIN) k.lin[i] = make_float4(r, g, b, 1.0f);
    if constexpr (RGBA) k.rgba8[i] = to8(r) | (to8(g) << 8) | (to8(b) << 16) | (255u << 24);
}

// ---- host side --------------------------------------------------------------------------
// What tells the two families apart on the host, beside Src: `noun` names the caller's record
// in the texts ("sky", "env"); `prep` is the record's input rule, which fills Src or sets the
// error and returns its status; `force64` is the family's process-wide debug flag and `path`
// the context's word for the address path of the family's last march (32 or 64).
template <class Src, class Rec>
using SkyPrep = vct_status (*)(vct_ctx* c, const char* what, const Rec& rec, Src& s);

// the grid and frame fields of a march record (SkyMarchK, SkySpecK); returns the block count
template <class K>
uint32_t march_fields(K& k, const Grid& g, bool o32, uint32_t w, uint32_t h) {
    alpha_ranges(g, o32, k.lvl);
    k.n = (int)g.n; k.L = (int)g.L; k.lgn = __builtin_ctz(g.n); k.aniso = g.aniso;
    k.w = (int)w; k.h = (int)h; k.tiles_x = (int)((w + 7) / 8);
    k.g0x = g.g0[0]; k.g0y = g.g0[1]; k.g0z = g.g0[2]; k.inv_h = g.inv_h;
    k.tmax = (float)g.n * VCT_SQRT3;
    return (uint32_t)k.tiles_x * ((h + 7) / 8);
}

// the receiver march over a w x h G-buffer, queued on the ctx stream; k.s is filled
template <class Src>
vct_status launch_march(vct_ctx* c, const char* what, SkyMarchK<Src>& k, const std::atomic<int>& force64, int* path,
                        const float4* pos, const float4* nrm, uint32_t w, uint32_t h, float4* sky4, float4* diff,
                        unsigned long long* cone_steps) {
    const Grid& g = c->grid;
    hipError_t e;
    const std::string name(what);
    k.nd = (int)c->cfg.n_diffuse;
    k.tau_set = k.nd == 16 ? VCT_TAN20 : VCT_TAN30;
    if (k.nd != 0) {
        // the diffuse aperture's table, from the context's set (ordered after its last march)
        uint8_t slot = 0;
        const StepRow* tabs = nullptr;
        if ((e = tables_enter(c)) != hipSuccess) return lhip(c, e, (name + ": stream wait").c_str());
        vct_status st = step_tables(c, what, &k.tau_set, 1, &slot, &tabs);
        if (st != VCT_OK) return st;
        k.tab = tabs + (size_t)slot * kShadowRows;
    }
    const bool o32 = g.n <= 512 && !force64.load();
    const uint32_t blocks = march_fields(k, g, o32, w, h);
    k.pos = pos; k.nrm = nrm;
    k.sky = sky4; k.diff = diff; k.steps_total = cone_steps;
    if (o32) hipLaunchKernelGGL((ksky_march<true, Src>), dim3(blocks), dim3(64), 0, c->stream, k);
    else hipLaunchKernelGGL((ksky_march<false, Src>), dim3(blocks), dim3(64), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, what);
    *path = o32 ? 32 : 64;
    if (k.nd != 0 && (e = tables_leave(c)) != hipSuccess) return lhip(c, e, (name + ": event record").c_str());
    return VCT_OK;
}

// vct_sky_cones_device / vct_env_cones_device after the context check
template <class Src, class Rec>
vct_status cones_call(vct_ctx* c, const char* what, const char* noun, const Rec* rec, SkyPrep<Src, Rec> prep,
                      const std::atomic<int>& force64, int* path, const float* pos4, const float* nrm4, uint32_t w,
                      uint32_t h, float* sky4, float* diffuse4_inout, unsigned long long* cone_steps) {
    const std::string name(what);
    if (!pos4 || !nrm4 || !sky4 || w == 0 || h == 0) return lfail(c, VCT_EINVAL, name + ": NULL buffer or empty frame");
    if (!rec) return lfail(c, VCT_EINVAL, name + ": NULL " + noun);
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, name + ": frame too large");
    if ((((uintptr_t)pos4 | (uintptr_t)nrm4 | (uintptr_t)sky4 | (uintptr_t)diffuse4_inout) & 15u) != 0)
        return lfail(c, VCT_EINVAL, name + ": float4 buffers must be 16-byte aligned");
    if (((uintptr_t)cone_steps & 7u) != 0) return lfail(c, VCT_EINVAL, name + ": cone_steps must be 8-byte aligned");
    SkyMarchK<Src> k;
    std::memset(&k, 0, sizeof k);
    vct_status st = prep(c, what, *rec, k.s);
    if (st != VCT_OK) return st;
    const Grid& g = c->grid;
    if (!g.voxelized || !g.mipped) return lfail(c, VCT_ESTATE, name + " before voxelize / build_mips");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    return launch_march(c, what, k, force64, path, (const float4*)pos4, (const float4*)nrm4, w, h, (float4*)sky4,
                        (float4*)diffuse4_inout, cone_steps);
}

// vct_inject_sky / vct_inject_env after the context check.  `skied`: the text for a level 0
// that already holds a sky.  `timed`: time the stages with the context's sky events
// (vct_debug_sky; the call then waits for its last stage).
template <class Src, class Rec>
vct_status inject_call(vct_ctx* c, const char* what, const char* noun, const Rec* rec, SkyPrep<Src, Rec> prep,
                       const std::atomic<int>& force64, int* path, const char* skied, bool timed) {
    const std::string name(what);
    if (!rec) return lfail(c, VCT_EINVAL, name + ": NULL " + noun);
    SkyMarchK<Src> k;
    std::memset(&k, 0, sizeof k);
    vct_status st = prep(c, what, *rec, k.s);
    if (st != VCT_OK) return st;
    Grid& g = c->grid;
    if (!g.voxelized) return lfail(c, VCT_ESTATE, name + " before voxelize");
    if (!g.injected || !g.mipped) return lfail(c, VCT_ESTATE, name + " before inject / build_mips");
    if (g.skied) return lfail(c, VCT_ESTATE, skied);
    if (g.bounced)
        return lfail(c, VCT_ESTATE, name + " after inject_bounces on this level 0 (the bounce's level 0 must "
                                           "already hold the sky)");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    if ((e = bounce_sources(c)) != hipSuccess) return lhip(c, e, (name + ": bounce sources").c_str());
    g.skied = true;
    const Bounce& b = c->bounce;
    // no cone (Sk = 0) or no source: level 0 and its mips stay as they are
    if (c->cfg.n_diffuse == 0 || b.n_src == 0) return VCT_OK;
    const std::string ev_record = name + ": event record";
    if (timed) {
        for (hipEvent_t& ev : c->sky_ev)
            if (!ev && (e = hipEventCreate(&ev)) != hipSuccess) return lhip(c, e, (name + ": event create").c_str());
        if ((e = hipEventRecord(c->sky_ev[0], c->stream)) != hipSuccess) return lhip(c, e, ev_record.c_str());
    }
    // Sk into the specular plane of the source G-buffer (K4's outputs: every gather writes
    // them before the accumulate reads them, so they are free here)
    constexpr int kPlane = 3;
    st = launch_march(c, what, k, force64, path, b.gbuf, b.gbuf + b.px_cap, b.tiles_x * VCT_TILE, b.tiles_y * VCT_TILE,
                      b.gbuf + (size_t)kPlane * b.px_cap, nullptr, nullptr);
    if (st != VCT_OK) return st;
    if (timed && (e = hipEventRecord(c->sky_ev[1], c->stream)) != hipSuccess) return lhip(c, e, ev_record.c_str());
    if ((e = launch_bounce_add_plane(c, kPlane)) != hipSuccess) return lhip(c, e, (name + ": add").c_str());
    if (timed && (e = hipEventRecord(c->sky_ev[2], c->stream)) != hipSuccess) return lhip(c, e, ev_record.c_str());
    g.mipped = false;
    g.l0_on_peers = false;   // device 0 added: vct_build_mips copies level 0 to the other devices
    // a relight build: level 0 is still nonzero exactly at the occupied voxels (alpha untouched)
    if ((st = vct_build_mips(c)) != VCT_OK) return st;
    if (timed) {
        if ((e = hipEventRecord(c->sky_ev[3], c->stream)) != hipSuccess ||
            (e = hipEventSynchronize(c->sky_ev[3])) != hipSuccess)
            return lhip(c, e, (name + ": event").c_str());
        for (int j = 0; j < 3; ++j)
            if ((e = hipEventElapsedTime(&c->sky_ms[j], c->sky_ev[j], c->sky_ev[j + 1])) != hipSuccess)
                return lhip(c, e, (name + ": event time").c_str());
    }
    return VCT_OK;
}

// vct_sky_specular_device / vct_env_specular_device after the context check
template <class Src, class Rec>
vct_status specular_call(vct_ctx* c, const char* what, const char* noun, const Rec* rec, SkyPrep<Src, Rec> prep,
                         const std::atomic<int>& force64, int* path, const float* pos4, const float* nrm4,
                         const float* alb4, uint32_t w, uint32_t h, const float* eye, float* skyspec4,
                         float* spec4_inout, unsigned long long* cone_steps) {
    const std::string name(what);
    if (!pos4 || !nrm4 || !alb4 || !skyspec4 || !eye || w == 0 || h == 0)
        return lfail(c, VCT_EINVAL, name + ": NULL buffer or empty frame");
    if (!rec) return lfail(c, VCT_EINVAL, name + ": NULL " + noun);
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, name + ": frame too large");
    if ((((uintptr_t)pos4 | (uintptr_t)nrm4 | (uintptr_t)alb4 | (uintptr_t)skyspec4 | (uintptr_t)spec4_inout) & 15u) != 0)
        return lfail(c, VCT_EINVAL, name + ": float4 buffers must be 16-byte aligned");
    if (((uintptr_t)cone_steps & 7u) != 0) return lfail(c, VCT_EINVAL, name + ": cone_steps must be 8-byte aligned");
    SkySpecK<Src> k;
    std::memset(&k, 0, sizeof k);
    vct_status st = prep(c, what, *rec, k.s);
    if (st != VCT_OK) return st;
    const Grid& g = c->grid;
    if (!g.voxelized || !g.mipped) return lfail(c, VCT_ESTATE, name + " before voxelize / build_mips");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    const bool o32 = g.n <= 512 && !force64.load();
    const uint32_t blocks = march_fields(k, g, o32, w, h);
    k.pos = (const float4*)pos4; k.nrm = (const float4*)nrm4; k.alb = (const float4*)alb4;
    k.out = (float4*)skyspec4; k.spec = (float4*)spec4_inout; k.steps_total = cone_steps;
    k.march = c->cfg.specular ? 1 : 0;
    k.ex = eye[0]; k.ey = eye[1]; k.ez = eye[2];
    if (o32) hipLaunchKernelGGL((ksky_spec<true, Src>), dim3(blocks), dim3(64), 0, c->stream, k);
    else hipLaunchKernelGGL((ksky_spec<false, Src>), dim3(blocks), dim3(64), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, what);
    *path = o32 ? 32 : 64;
    return VCT_OK;
}

// vct_sky_background_device / vct_env_background_device after the context check
template <class Src, class Rec>
vct_status background_call(vct_ctx* c, const char* what, const char* noun, const Rec* rec, SkyPrep<Src, Rec> prep,
                           const vct_camera* cam, const float* pos4, uint32_t w, uint32_t h, float* linear4_inout,
                           uint32_t* rgba8_inout) {
    const std::string name(what);
    if (!cam || !pos4 || w == 0 || h == 0) return lfail(c, VCT_EINVAL, name + ": NULL camera, NULL buffer or empty frame");
    if (!rec) return lfail(c, VCT_EINVAL, name + ": NULL " + noun);
    if (!linear4_inout && !rgba8_inout) return lfail(c, VCT_EINVAL, name + ": no output");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, name + ": frame too large");
    if ((((uintptr_t)pos4 | (uintptr_t)linear4_inout) & 15u) != 0)
        return lfail(c, VCT_EINVAL, name + ": float4 buffers must be 16-byte aligned");
    if (((uintptr_t)rgba8_inout & 3u) != 0) return lfail(c, VCT_EINVAL, name + ": rgba8 buffer must be 4-byte aligned");
    SkyBgK<Src> k;
    std::memset(&k, 0, sizeof k);
    vct_status st = prep(c, what, *rec, k.s);
    if (st != VCT_OK) return st;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    camera_fields(k, cam, w, h);
    k.pos = (const float4*)pos4; k.lin = (float4*)linear4_inout; k.rgba8 = rgba8_inout; k.npx = w * h;
    const dim3 grid((k.npx + 255) / 256), block(256);
    if (k.lin && k.rgba8) hipLaunchKernelGGL((ksky_bg<true, true, Src>), grid, block, 0, c->stream, k);
    else if (k.lin) hipLaunchKernelGGL((ksky_bg<true, false, Src>), grid, block, 0, c->stream, k);
    else hipLaunchKernelGGL((ksky_bg<false, true, Src>), grid, block, 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, what);
    return VCT_OK;
}

}  // namespace
}  // namespace vct
