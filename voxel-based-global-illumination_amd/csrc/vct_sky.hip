// vct_sky.hip — sky light (include/vct_sky.h; the arithmetic is include/vct_spec.h "sky
// light"): the context's diffuse cone set marched through the alpha of the pyramid for every
// receiver, each cone weighting the sky colour of its direction by the transmittance it ends
// with.  One kernel serves the pixels of a frame (vct_sky_cones_device) and the bounce
// sources of a voxelization (vct_inject_sky): vct_bounce.hip keeps the sources as a
// materialised G-buffer in which every aligned 8x8 block holds 64 neighbouring sources, so
// the frame kernel runs on it unchanged.
//
//   ksky_march   the work shape of ks_march (vct_shadow.hip): one wave per 8x8 block, one
//                lane per record.  The cone loop is wave-uniform and in set order, so every
//                receiver's fmaf chain is its lane's own, in the spec's order, without an
//                atomic.  Each cone is vct_alpha_march.h's lockstep march with t_lim = +inf:
//                step i is the same (t, D, l0, fr) for every lane, an ended lane only drops
//                out of a mask with its loads sent past the buffer range, and the loop ends
//                on a ballot.  The directions (K4's tangent frame of the lane's normal) are
//                per lane, so the faces and d^2 are per lane, as for ks_march's point lights.
//   k_bounce_add_plane (vct_bounce.hip)  level 0 += A * Sk at every source.
//
// Addresses: every texel offset is built from integers that were range-checked against the
// level (vct_alpha_march.h axis_fields): on the O32 path a corner outside its level, and
// every corner of an ended lane, becomes an offset past the bound range, which the hardware
// range check answers with zero; the 64-bit path reads texel 0 instead and selects zero.  A
// non-finite p fails the inside test, so a pixel with a non-finite position or normal ends
// its cones before the first sample.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstring>
#include "vct_internal.h"
#include "vct_light_terms.h"
#include "vct_alpha_march.h"

namespace vct {
namespace {

static_assert(sizeof(vct_sky) == 48, "vct_sky is 12 floats (include/vct_sky.h)");

struct SkyK {
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
    float ux, uy, uz;            // up_n
    float zr, zg, zb, hr, hg, hb, gr, gg, gb;
};

#define VCT_SKY_ROW(cn, ct, cb, w) {cn, ct, cb, w},
__device__ const float kSkyCones1[1][4] = {VCT_CONES1(VCT_SKY_ROW)};
__device__ const float kSkyCones9[9][4] = {VCT_CONES9(VCT_SKY_ROW)};
__device__ const float kSkyCones16[16][4] = {VCT_CONES16(VCT_SKY_ROW)};
#undef VCT_SKY_ROW

template <bool O32>
__global__ void __launch_bounds__(64) ksky_march(const SkyK k) {
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
    // K4's tangent frame (A.5; Duff et al. 2017), the operations in K4's order
    const float sgn = copysignf(1.0f, nz);
    const float ka = -1.0f / (sgn + nz);
    const float kb = (nx * ny) * ka;
    const float Tx = 1.0f + ((sgn * nx) * nx) * ka, Ty = sgn * kb, Tz = -(sgn * nx);
    const float Bx = kb, By = sgn + (ny * ny) * ka, Bz = -ny;
    const float(*cones)[4] = k.nd == 16 ? kSkyCones16 : (k.nd == 9 ? kSkyCones9 : kSkyCones1);
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, vis = 0.0f;
    uint32_t steps = 0;
    for (int c = 0; c < k.nd; ++c) {
        const float cn = cones[c][0], ct = cones[c][1], cb = cones[c][2], wk = cones[c][3];
        const float dx = (cn * nx + ct * Tx) + cb * Bx;
        const float dy = (cn * ny + ct * Ty) + cb * By;
        const float dz = (cn * nz + ct * Tz) + cb * Bz;
        const float a = cone<O32>(k, k.tab, valid, ox, oy, oz, dx, dy, dz, __builtin_inff(), steps);
        const float T = fmaxf(1.0f - a / VCT_ALPHA_STOP, 0.0f);
        const float u = dot3(dx, dy, dz, k.ux, k.uy, k.uz);
        const float s_up = fminf(fmaxf(u, 0.0f), 1.0f), s_dn = fminf(fmaxf(-u, 0.0f), 1.0f);
        const float sr = (k.hr + (k.zr - k.hr) * s_up) + (k.gr - k.hr) * s_dn;
        const float sg = (k.hg + (k.zg - k.hg) * s_up) + (k.gg - k.hg) * s_dn;
        const float sb = (k.hb + (k.zb - k.hb) * s_up) + (k.gb - k.hb) * s_dn;
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

// ---- host side --------------------------------------------------------------------------
std::atomic<int> g_sky_force64{0};   // vct_debug_sky: every grid takes the 64-bit path

// the input rule of vct_spec.h "sky light": up by the K2 direction rule, the colours by the K2
// colour rule; fills k's sky constants, or returns what is wrong
const char* prepare_sky(const vct_sky& in, SkyK& k) {
    const float ux = in.up[0], uy = in.up[1], uz = in.up[2];
    const float len = sqrtf((ux * ux + uy * uy) + uz * uz);
    if (!(len > 0.0f) || !std::isfinite(len)) return "zero or non-finite up";
    if (const char* bad = check_color(in.zenith)) return bad;
    if (const char* bad = check_color(in.horizon)) return bad;
    if (const char* bad = check_color(in.ground)) return bad;
    k.ux = ux / len; k.uy = uy / len; k.uz = uz / len;
    k.zr = in.zenith[0]; k.zg = in.zenith[1]; k.zb = in.zenith[2];
    k.hr = in.horizon[0]; k.hg = in.horizon[1]; k.hb = in.horizon[2];
    k.gr = in.ground[0]; k.gg = in.ground[1]; k.gb = in.ground[2];
    return nullptr;
}

// the march over a w x h G-buffer, queued on the ctx stream; k holds the sky constants
vct_status sky_march(vct_ctx* c, const char* what, SkyK& k, const float4* pos, const float4* nrm, uint32_t w,
                     uint32_t h, float4* sky4, float4* diff, unsigned long long* cone_steps) {
    const Grid& g = c->grid;
    hipError_t e;
    const std::string name(what);
    k.nd = (int)c->cfg.n_diffuse;
    if (k.nd != 0) {
        // the diffuse aperture's table, from the context's set (ordered after its last march)
        const float tau = k.nd == 16 ? VCT_TAN20 : VCT_TAN30;
        uint8_t slot = 0;
        const StepRow* tabs = nullptr;
        if ((e = tables_enter(c)) != hipSuccess) return lhip(c, e, (name + ": stream wait").c_str());
        vct_status st = step_tables(c, what, &tau, 1, &slot, &tabs);
        if (st != VCT_OK) return st;
        k.tab = tabs + (size_t)slot * kShadowRows;
    }
    const bool o32 = g.n <= 512 && !g_sky_force64.load();
    alpha_ranges(g, o32, k.lvl);
    k.pos = pos; k.nrm = nrm;
    k.sky = sky4; k.diff = diff; k.steps_total = cone_steps;
    k.n = (int)g.n; k.L = (int)g.L; k.lgn = __builtin_ctz(g.n); k.aniso = g.aniso;
    k.w = (int)w; k.h = (int)h; k.tiles_x = (int)((w + 7) / 8);
    k.g0x = g.g0[0]; k.g0y = g.g0[1]; k.g0z = g.g0[2]; k.inv_h = g.inv_h;
    k.tmax = (float)g.n * VCT_SQRT3;
    const uint32_t blocks = (uint32_t)k.tiles_x * ((h + 7) / 8);
    if (o32) hipLaunchKernelGGL(ksky_march<true>, dim3(blocks), dim3(64), 0, c->stream, k);
    else hipLaunchKernelGGL(ksky_march<false>, dim3(blocks), dim3(64), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, what);
    c->sky_path = o32 ? 32 : 64;
    if (k.nd != 0 && (e = tables_leave(c)) != hipSuccess) return lhip(c, e, (name + ": event record").c_str());
    return VCT_OK;
}

}  // namespace
}  // namespace vct

using namespace vct;

extern "C" vct_status vct_sky_cones_device(vct_ctx* c, const float* pos4, const float* nrm4, uint32_t w, uint32_t h,
                                           const vct_sky* sky, float* sky4, float* diffuse4_inout,
                                           unsigned long long* cone_steps) {
    if (!c) return VCT_EINVAL;
    if (!pos4 || !nrm4 || !sky4 || w == 0 || h == 0) return lfail(c, VCT_EINVAL, "sky_cones: NULL buffer or empty frame");
    if (!sky) return lfail(c, VCT_EINVAL, "sky_cones: NULL sky");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "sky_cones: frame too large");
    if ((((uintptr_t)pos4 | (uintptr_t)nrm4 | (uintptr_t)sky4 | (uintptr_t)diffuse4_inout) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "sky_cones: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)cone_steps & 7u) != 0) return lfail(c, VCT_EINVAL, "sky_cones: cone_steps must be 8-byte aligned");
    SkyK k;
    std::memset(&k, 0, sizeof k);
    if (const char* bad = prepare_sky(*sky, k)) return lfail(c, VCT_EINVAL, std::string("sky_cones: ") + bad);
    const Grid& g = c->grid;
    if (!g.voxelized || !g.mipped) return lfail(c, VCT_ESTATE, "sky_cones before voxelize / build_mips");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    return sky_march(c, "sky_cones", k, (const float4*)pos4, (const float4*)nrm4, w, h, (float4*)sky4,
                     (float4*)diffuse4_inout, cone_steps);
}

extern "C" vct_status vct_inject_sky(vct_ctx* c, const vct_sky* sky) {
    if (!c) return VCT_EINVAL;
    if (!sky) return lfail(c, VCT_EINVAL, "inject_sky: NULL sky");
    SkyK k;
    std::memset(&k, 0, sizeof k);
    if (const char* bad = prepare_sky(*sky, k)) return lfail(c, VCT_EINVAL, std::string("inject_sky: ") + bad);
    Grid& g = c->grid;
    if (!g.voxelized) return lfail(c, VCT_ESTATE, "inject_sky before voxelize");
    if (!g.injected || !g.mipped) return lfail(c, VCT_ESTATE, "inject_sky before inject / build_mips");
    if (g.skied) return lfail(c, VCT_ESTATE, "inject_sky twice on one level 0 (inject or upload a new one first)");
    if (g.bounced)
        return lfail(c, VCT_ESTATE, "inject_sky after inject_bounces on this level 0 (the bounce's level 0 must "
                                    "already hold the sky)");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    if ((e = bounce_sources(c)) != hipSuccess) return lhip(c, e, "inject_sky: bounce sources");
    g.skied = true;
    const Bounce& b = c->bounce;
    // no cone (Sk = 0) or no source: level 0 and its mips stay as they are
    if (c->cfg.n_diffuse == 0 || b.n_src == 0) return VCT_OK;
    const bool timed = c->sky_profile;
    if (timed) {
        for (hipEvent_t& ev : c->sky_ev)
            if (!ev && (e = hipEventCreate(&ev)) != hipSuccess) return lhip(c, e, "inject_sky: event create");
        if ((e = hipEventRecord(c->sky_ev[0], c->stream)) != hipSuccess) return lhip(c, e, "inject_sky: event record");
    }
    // Sk into the specular plane of the source G-buffer (K4's outputs: every gather writes
    // them before the accumulate reads them, so they are free here)
    constexpr int kPlane = 3;
    vct_status st = sky_march(c, "inject_sky", k, b.gbuf, b.gbuf + b.px_cap, b.tiles_x * VCT_TILE, b.tiles_y * VCT_TILE,
                              b.gbuf + (size_t)kPlane * b.px_cap, nullptr, nullptr);
    if (st != VCT_OK) return st;
    if (timed && (e = hipEventRecord(c->sky_ev[1], c->stream)) != hipSuccess) return lhip(c, e, "inject_sky: event record");
    if ((e = launch_bounce_add_plane(c, kPlane)) != hipSuccess) return lhip(c, e, "inject_sky: add");
    if (timed && (e = hipEventRecord(c->sky_ev[2], c->stream)) != hipSuccess) return lhip(c, e, "inject_sky: event record");
    g.mipped = false;
    g.l0_on_peers = false;   // device 0 added: vct_build_mips copies level 0 to the other devices
    // a relight build: level 0 is still nonzero exactly at the occupied voxels (alpha untouched)
    if ((st = vct_build_mips(c)) != VCT_OK) return st;
    if (timed) {
        if ((e = hipEventRecord(c->sky_ev[3], c->stream)) != hipSuccess ||
            (e = hipEventSynchronize(c->sky_ev[3])) != hipSuccess)
            return lhip(c, e, "inject_sky: event");
        for (int j = 0; j < 3; ++j)
            if ((e = hipEventElapsedTime(&c->sky_ms[j], c->sky_ev[j], c->sky_ev[j + 1])) != hipSuccess)
                return lhip(c, e, "inject_sky: event time");
    }
    return VCT_OK;
}

// Test and tool hook (not part of the public headers).  force64 >= 0: nonzero sends every
// grid's sky march through the 64-bit-address path that 1024^3 takes (process-wide).
// profile >= 0 (with a context): nonzero times the stages of the following vct_inject_sky
// calls with events (the call then waits for its last stage).  ms3 (nullable) receives the
// march, add and K3 times of the last timed vct_inject_sky.
extern "C" int vct_debug_sky(vct_ctx* c, int force64, int profile, float* ms3) {
    if (force64 >= 0) g_sky_force64.store(force64 ? 1 : 0);
    if (c && profile >= 0) c->sky_profile = profile != 0;
    if (c && ms3)
        for (int i = 0; i < 3; ++i) ms3[i] = c->sky_ms[i];
    return 0;
}

// The address path the context's last sky march was launched with: 32 (buffer resources), 64
// (64-bit addresses), 0 before the first one.
extern "C" int vct_debug_sky_path(const vct_ctx* c) { return c ? c->sky_path : -1; }
