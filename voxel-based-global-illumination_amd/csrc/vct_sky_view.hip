// vct_sky_view.hip — the sky in view (include/vct_sky_view.h; the arithmetic is
// include/vct_spec.h "sky in view"): the sky in the specular cone of every pixel, and the sky
// behind the scene.
//
//   ksky_spec   the work shape of ksky_march (vct_sky.hip): one wave per 8x8 block, one lane
//               per pixel.  The cone is K4's specular cone reduced to its alpha channel; its
//               aperture is the pixel's roughness, so every lane derives its own steps in
//               registers (t, D = max(1, 2 tau t), m = log2 D, l0, fr: K4's per-lane march)
//               and no step table is involved.  vct_alpha_march.h's sample_alpha wants a
//               wave-uniform level, so a step loops over the levels present among the lanes
//               that still march: the first pending lane's l0 is read onto the scalar unit,
//               the lanes of that level sample and leave the pending mask.  A wave whose
//               pixels share one roughness has one t sequence and runs the loop once per step
//               (the lockstep march, with no special case); a wave of mixed roughness pays
//               one pass per distinct level.  The second level of a step (fr > 0, l0 < L) is
//               handled the same way.  A lane outside the pass has its loads sent past the
//               buffer range (O32) or reads texel 0 and selects zero (64-bit), as an ended
//               lane of the lockstep march does.
//   ksky_bg     a streaming kernel: one float4 load of pos4 per pixel, stores at background
//               pixels only, compiled once per set of outputs.
//
// Every pixel is one lane's own, so the only atomic is the wave-summed step counter.  A
// non-finite reflected direction fails the inside test before the first sample.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstring>
#include "vct_internal.h"
#include "vct_light_terms.h"
#include "vct_alpha_march.h"
#include "vct_view.h"

namespace vct {
namespace {

// the constants of Sky(d) ("sky light"): up_n and the three colours
struct SkyColors {
    float ux, uy, uz;
    float zr, zg, zb, hr, hg, hb, gr, gg, gb;
};

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
    SkyColors s;
};

struct SkyBgK {
    const float4* pos;
    float4* lin;
    uint32_t* rgba8;
    uint32_t npx;
    int w, h;
    float fx, fy, fz, ux, uy, uz, rx, ry, rz, tan_half, aspect;   // vct_view.h camera_fields
    SkyColors s;
};

__device__ __forceinline__ void sky_of(const SkyColors& s, float dx, float dy, float dz, float& r, float& g, float& b) {
    const float u = dot3(dx, dy, dz, s.ux, s.uy, s.uz);
    const float s_up = fminf(fmaxf(u, 0.0f), 1.0f), s_dn = fminf(fmaxf(-u, 0.0f), 1.0f);
    r = (s.hr + (s.zr - s.hr) * s_up) + (s.gr - s.hr) * s_dn;
    g = (s.hg + (s.zg - s.hg) * s_up) + (s.gg - s.hg) * s_dn;
    b = (s.hb + (s.zb - s.hb) * s_up) + (s.gb - s.hb) * s_dn;
}

template <bool O32>
__global__ void __launch_bounds__(64) ksky_spec(const SkySpecK k) {
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
    // A.6's specular cone, the operations in K4's order
    float vx = k.ex - P.x, vy = k.ey - P.y, vz = k.ez - P.z;
    const float vl = sqrtf(dot3(vx, vy, vz, vx, vy, vz));
    vx = vx / vl; vy = vy / vl; vz = vz / vl;
    const float ndv = dot3(nx, ny, nz, vx, vy, vz);
    const float k2 = 2.0f * ndv;
    const float dx = k2 * nx - vx, dy = k2 * ny - vy, dz = k2 * nz - vz;
    const float tau = fminf(fmaxf(rough, VCT_SPEC_TAU_MIN), VCT_SPEC_TAU_MAX);
    const float tau2 = 2.0f * tau;

    const float nf = (float)k.n, Lf = (float)k.L;
    const int fx = dx >= 0.0f ? VCT_FACE_PX : VCT_FACE_NX;
    const int fy = dy >= 0.0f ? VCT_FACE_PY : VCT_FACE_NY;
    const int fz = dz >= 0.0f ? VCT_FACE_PZ : VCT_FACE_NZ;
    const float wdx = dx * dx, wdy = dy * dy, wdz = dz * dz;
    float a = 0.0f, t = 1.0f;
    bool act = valid;
    uint32_t steps = 0;
    for (;;) {
        // "shadow cones" step 1, t_lim = +inf; t grows by at least 0.5 a step, so the loop ends
        const float px = ox + dx * t, py = oy + dy * t, pz = oz + dz * t;
        act = act & (a < VCT_ALPHA_STOP) & (t <= k.tmax) &
              ((px >= 0.0f) & (px <= nf) & (py >= 0.0f) & (py <= nf) & (pz >= 0.0f) & (pz <= nf));
        const unsigned long long am = __builtin_amdgcn_ballot_w64(act);
        if (am == 0ull) break;
        // step 2, per lane (tau is clamped and t <= tmax on a marching lane: 0 <= m <= L)
        const float D = fmaxf(1.0f, tau2 * t);
        const float m = fminf(spec_log2(D), Lf);
        const int l0 = act ? (int)m : 0;
        const float fr = m - (float)l0;
        // step 3: one pass per level present among the marching lanes
        float s = 0.0f;
        for (unsigned long long pend = am; pend != 0ull;) {
            const int l = __builtin_amdgcn_readlane(l0, __builtin_ctzll(pend));
            const bool mine = act & (l0 == l);
            const float v = sample_alpha<O32>(k, l, mine, px, py, pz, fx, fy, fz, wdx, wdy, wdz);
            s = mine ? v : s;
            pend &= ~__builtin_amdgcn_ballot_w64(mine);
        }
        // step 4: the same over the lanes that blend in level l0 + 1
        const bool two = act & (fr > 0.0f) & (l0 < k.L);
        float s1 = 0.0f;
        for (unsigned long long pend = __builtin_amdgcn_ballot_w64(two); pend != 0ull;) {
            const int l = __builtin_amdgcn_readlane(l0, __builtin_ctzll(pend));
            const bool mine = two & (l0 == l);
            const float v = sample_alpha<O32>(k, l + 1, mine, px, py, pz, fx, fy, fz, wdx, wdy, wdz);
            s1 = mine ? v : s1;
            pend &= ~__builtin_amdgcn_ballot_w64(mine);
        }
        s = two ? fmaf(fr, s1, (1.0f - fr) * s) : s;
        // step 5
        const float oma = 1.0f - a;
        a = act ? fmaf(oma, s, a) : a;
        steps += act ? 1u : 0u;
        t = t + VCT_STEP_SCALE * D;
    }
    if (inframe) {
        const float T = fmaxf(1.0f - a / VCT_ALPHA_STOP, 0.0f);
        float sr, sg, sb;
        sky_of(k.s, dx, dy, dz, sr, sg, sb);
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

template <bool LIN, bool RGBA>
__global__ void __launch_bounds__(256) ksky_bg(const SkyBgK k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k.npx) return;
    const float4 P = k.pos[i];
    if (P.w != 0.0f) return;
    const int y = (int)(i / (uint32_t)k.w), x = (int)(i - (uint32_t)y * (uint32_t)k.w);
    float dx, dy, dz, r, g, b;
    pixel_ray(k, x, y, dx, dy, dz);
    sky_of(k.s, dx, dy, dz, r, g, b);
    if constexpr (LIN) k.lin[i] = make_float4(r, g, b, 1.0f);
    if constexpr (RGBA) k.rgba8[i] = to8(r) | (to8(g) << 8) | (to8(b) << 16) | (255u << 24);
}

// ---- host side --------------------------------------------------------------------------
std::atomic<int> g_sky_view_force64{0};   // vct_debug_sky_view: every grid takes the 64-bit path

// the input rule of vct_spec.h "sky light": up by the K2 direction rule, the colours by the K2
// colour rule; fills the sky constants, or returns what is wrong
const char* prepare_colors(const vct_sky& in, SkyColors& s) {
    const float ux = in.up[0], uy = in.up[1], uz = in.up[2];
    const float len = sqrtf((ux * ux + uy * uy) + uz * uz);
    if (!(len > 0.0f) || !std::isfinite(len)) return "zero or non-finite up";
    if (const char* bad = check_color(in.zenith)) return bad;
    if (const char* bad = check_color(in.horizon)) return bad;
    if (const char* bad = check_color(in.ground)) return bad;
    s.ux = ux / len; s.uy = uy / len; s.uz = uz / len;
    s.zr = in.zenith[0]; s.zg = in.zenith[1]; s.zb = in.zenith[2];
    s.hr = in.horizon[0]; s.hg = in.horizon[1]; s.hb = in.horizon[2];
    s.gr = in.ground[0]; s.gg = in.ground[1]; s.gb = in.ground[2];
    return nullptr;
}

}  // namespace
}  // namespace vct

using namespace vct;

extern "C" vct_status vct_sky_specular_device(vct_ctx* c, const float* pos4, const float* nrm4, const float* alb4,
                                              uint32_t w, uint32_t h, const float* eye, const vct_sky* sky,
                                              float* skyspec4, float* spec4_inout, unsigned long long* cone_steps) {
    if (!c) return VCT_EINVAL;
    if (!pos4 || !nrm4 || !alb4 || !skyspec4 || !eye || w == 0 || h == 0)
        return lfail(c, VCT_EINVAL, "sky_specular: NULL buffer or empty frame");
    if (!sky) return lfail(c, VCT_EINVAL, "sky_specular: NULL sky");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "sky_specular: frame too large");
    if ((((uintptr_t)pos4 | (uintptr_t)nrm4 | (uintptr_t)alb4 | (uintptr_t)skyspec4 | (uintptr_t)spec4_inout) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "sky_specular: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)cone_steps & 7u) != 0) return lfail(c, VCT_EINVAL, "sky_specular: cone_steps must be 8-byte aligned");
    SkySpecK k;
    std::memset(&k, 0, sizeof k);
    if (const char* bad = prepare_colors(*sky, k.s)) return lfail(c, VCT_EINVAL, std::string("sky_specular: ") + bad);
    const Grid& g = c->grid;
    if (!g.voxelized || !g.mipped) return lfail(c, VCT_ESTATE, "sky_specular before voxelize / build_mips");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    const bool o32 = g.n <= 512 && !g_sky_view_force64.load();
    alpha_ranges(g, o32, k.lvl);
    k.pos = (const float4*)pos4; k.nrm = (const float4*)nrm4; k.alb = (const float4*)alb4;
    k.out = (float4*)skyspec4; k.spec = (float4*)spec4_inout; k.steps_total = cone_steps;
    k.n = (int)g.n; k.L = (int)g.L; k.lgn = __builtin_ctz(g.n); k.aniso = g.aniso;
    k.w = (int)w; k.h = (int)h; k.tiles_x = (int)((w + 7) / 8);
    k.march = c->cfg.specular ? 1 : 0;
    k.g0x = g.g0[0]; k.g0y = g.g0[1]; k.g0z = g.g0[2]; k.inv_h = g.inv_h;
    k.tmax = (float)g.n * VCT_SQRT3;
    k.ex = eye[0]; k.ey = eye[1]; k.ez = eye[2];
    const uint32_t blocks = (uint32_t)k.tiles_x * ((h + 7) / 8);
    if (o32) hipLaunchKernelGGL(ksky_spec<true>, dim3(blocks), dim3(64), 0, c->stream, k);
    else hipLaunchKernelGGL(ksky_spec<false>, dim3(blocks), dim3(64), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "sky_specular");
    c->sky_view_path = o32 ? 32 : 64;
    return VCT_OK;
}

extern "C" vct_status vct_sky_background_device(vct_ctx* c, const vct_camera* cam, const float* pos4, uint32_t w,
                                                uint32_t h, const vct_sky* sky, float* linear4_inout,
                                                uint32_t* rgba8_inout) {
    if (!c) return VCT_EINVAL;
    if (!cam || !pos4 || w == 0 || h == 0) return lfail(c, VCT_EINVAL, "sky_background: NULL camera, NULL buffer or empty frame");
    if (!sky) return lfail(c, VCT_EINVAL, "sky_background: NULL sky");
    if (!linear4_inout && !rgba8_inout) return lfail(c, VCT_EINVAL, "sky_background: no output");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "sky_background: frame too large");
    if ((((uintptr_t)pos4 | (uintptr_t)linear4_inout) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "sky_background: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)rgba8_inout & 3u) != 0) return lfail(c, VCT_EINVAL, "sky_background: rgba8 buffer must be 4-byte aligned");
    SkyBgK k;
    std::memset(&k, 0, sizeof k);
    if (const char* bad = prepare_colors(*sky, k.s)) return lfail(c, VCT_EINVAL, std::string("sky_background: ") + bad);
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    camera_fields(k, cam, w, h);
    k.pos = (const float4*)pos4; k.lin = (float4*)linear4_inout; k.rgba8 = rgba8_inout; k.npx = w * h;
    const dim3 grid((k.npx + 255) / 256), block(256);
    if (k.lin && k.rgba8) hipLaunchKernelGGL((ksky_bg<true, true>), grid, block, 0, c->stream, k);
    else if (k.lin) hipLaunchKernelGGL((ksky_bg<true, false>), grid, block, 0, c->stream, k);
    else hipLaunchKernelGGL((ksky_bg<false, true>), grid, block, 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "sky_background");
    return VCT_OK;
}

// Test and tool hook (not part of the public headers).  force64 >= 0: nonzero sends every
// grid's specular sky march through the 64-bit-address path that 1024^3 takes (process-wide).
extern "C" int vct_debug_sky_view(int force64) {
    if (force64 >= 0) g_sky_view_force64.store(force64 ? 1 : 0);
    return 0;
}

// The address path the context's last specular sky march was launched with: 32 (buffer
// resources), 64 (64-bit addresses), 0 before the first one.
extern "C" int vct_debug_sky_view_path(const vct_ctx* c) { return c ? c->sky_view_path : -1; }
