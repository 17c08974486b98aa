// vct_env.hip — the environment-map sky (include/vct_env.h; the arithmetic is
// include/vct_spec.h "environment sky"): an octahedral HDR map with its mip chain in the
// context, Env(d, tau) looked up by direction and aperture, and the four sky calls with that
// colour in the place of Sky(d).
//
//   kenv_mip     one thread per texel of level j + 1: the 2 x 2 box of level j.
//   env_color    the lookup, per lane: the octahedral point of the direction, the level pair of
//                the aperture, and two bilinear samples -- eight float4 gathers, all addressed
//                before the first is used, so they are in flight together.  Every tap index is
//                clamped to its level before it becomes an address (the fold rule clamps
//                anyway), and a lane without a second level gathers the first one twice, so no
//                lane reads outside the pyramid whatever its direction and aperture hold.  A
//                degenerate direction becomes the one texel of the last level the same way
//                (level lg S, p = 0), without a branch around the gathers.
//   kenv_lookup  env_color for one (d, tau) per lane (vct_env_lookup_device).
//   kenv_march   ksky_march (vct_sky.hip) with env_color for the colour: one wave per 8x8
//                block, one lane per record, the cones in set order through
//                vct_alpha_march.h's lockstep cone<>.  The set's aperture is wave-uniform, so
//                the level pair of the lookup is too; the taps are per lane.
//   kenv_spec    ksky_spec (vct_sky_view.hip) restated, with env_color at the pixel's own
//                aperture: the level pair is per lane.
//   kenv_bg      ksky_bg with Env(d, 0).
//
// The marches are the sky kernels' line for line (vct_sky.hip and vct_sky_view.hip say how
// their addresses stay in range); the only new addresses are env_color's.
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

static_assert(sizeof(vct_env_sky) == 40, "vct_env_sky is 10 floats (include/vct_env.h)");

// the map and the record, as every kernel here takes them
struct EnvMapK {
    const float4* map;
    uint32_t s2;                 // S * S
    int lg;                      // lg S
    float Sf, lgf;               // (float)S, (float)lg S
    float f[3][3];
    float scale;
};

// first texel of level j (S_j = S >> j): the levels lie back to back
__host__ __device__ __forceinline__ uint32_t env_level_off(uint32_t s2, uint32_t sj) {
    return 4u * (s2 - sj * sj) / 3u;
}

struct EnvTaps {
    uint32_t a, b, c, d;
    float fu, fv;
};

// step 4's taps of level j at p (|p_c| <= 1): texel indices into the pyramid, fold rule applied
__device__ __forceinline__ EnvTaps env_taps(const EnvMapK& e, int j, float px, float py) {
    const int sj = 1 << (e.lg - j), hi = sj - 1;
    const float sjf = (float)sj;
    const float u = (px * 0.5f + 0.5f) * sjf - 0.5f, v = (py * 0.5f + 0.5f) * sjf - 0.5f;
    const float fi = floorf(u), fk = floorf(v);
    const int i0 = min(max((int)fi, -1), hi), k0 = min(max((int)fk, -1), hi);
    const int x0 = max(i0, 0), x1 = min(i0 + 1, hi), y0 = max(k0, 0), y1 = min(k0 + 1, hi);
    const bool ox0 = i0 < 0, ox1 = i0 + 1 > hi, oy0 = k0 < 0, oy1 = k0 + 1 > hi;
    const uint32_t off = env_level_off(e.s2, (uint32_t)sj);
    const auto tap = [&](int x, bool ox, int y, bool oy) {
        const int row = ox ? hi - y : y, col = oy ? hi - x : x;
        return off + (uint32_t)row * (uint32_t)sj + (uint32_t)col;
    };
    return EnvTaps{tap(x0, ox0, y0, oy0), tap(x1, ox1, y0, oy0), tap(x0, ox0, y1, oy1), tap(x1, ox1, y1, oy1),
                   u - fi, v - fk};
}

__device__ __forceinline__ float env_bilinear(float a, float b, float c, float d, float fu, float fv) {
    const float t0 = fmaf(fu, b - a, a), t1 = fmaf(fu, d - c, c);
    return fmaf(fv, t1 - t0, t0);
}

// Env(d, tau) -> r, g, b; returns the level m of step 3
__device__ __forceinline__ float env_color(const EnvMapK& e, float dx, float dy, float dz, float tau, float& r, float& g,
                                           float& b) {
    const float ex = dot3(e.f[0][0], e.f[0][1], e.f[0][2], dx, dy, dz);
    const float ey = dot3(e.f[1][0], e.f[1][1], e.f[1][2], dx, dy, dz);
    const float ez = dot3(e.f[2][0], e.f[2][1], e.f[2][2], dx, dy, dz);
    const float s = (fabsf(ex) + fabsf(ey)) + fabsf(ez);
    const bool ok = (s > 0.0f) & (s < __builtin_inff());
    float px = ex / s, py = ey / s;
    if (ez < 0.0f) {
        const float qx = (1.0f - fabsf(py)) * copysignf(1.0f, px), qy = (1.0f - fabsf(px)) * copysignf(1.0f, py);
        px = qx; py = qy;
    }
    const float x = fminf(fmaxf(tau * e.Sf, 1.0f), e.Sf);
    const float m = fminf(spec_log2(x), e.lgf);
    int j0 = (int)m;
    float fr = m - (float)j0;
    if (!ok) { j0 = e.lg; fr = 0.0f; px = 0.0f; py = 0.0f; }   // the map's mean: S_j = 1, every tap texel (0, 0)
    j0 = min(max(j0, 0), e.lg);
    const bool two = (fr > 0.0f) & (j0 < e.lg);
    const EnvTaps t0 = env_taps(e, j0, px, py), t1 = env_taps(e, two ? j0 + 1 : j0, px, py);
    const float4 a0 = e.map[t0.a], b0 = e.map[t0.b], c0 = e.map[t0.c], d0 = e.map[t0.d];
    const float4 a1 = e.map[t1.a], b1 = e.map[t1.b], c1 = e.map[t1.c], d1 = e.map[t1.d];
    const float r0 = env_bilinear(a0.x, b0.x, c0.x, d0.x, t0.fu, t0.fv);
    const float g0 = env_bilinear(a0.y, b0.y, c0.y, d0.y, t0.fu, t0.fv);
    const float bl0 = env_bilinear(a0.z, b0.z, c0.z, d0.z, t0.fu, t0.fv);
    const float r1 = env_bilinear(a1.x, b1.x, c1.x, d1.x, t1.fu, t1.fv);
    const float g1 = env_bilinear(a1.y, b1.y, c1.y, d1.y, t1.fu, t1.fv);
    const float bl1 = env_bilinear(a1.z, b1.z, c1.z, d1.z, t1.fu, t1.fv);
    r = (two ? fmaf(fr, r1 - r0, r0) : r0) * e.scale;
    g = (two ? fmaf(fr, g1 - g0, g0) : g0) * e.scale;
    b = (two ? fmaf(fr, bl1 - bl0, bl0) : bl0) * e.scale;
    return m;
}

__global__ void __launch_bounds__(256) kenv_mip(const float4* __restrict__ src, float4* __restrict__ dst, uint32_t sd) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= sd * sd) return;
    const uint32_t y = i / sd, x = i - y * sd, ss = 2u * sd;
    const float4* r0 = src + (size_t)(2u * y) * ss + 2u * x;
    const float4 a00 = r0[0], a10 = r0[1], a01 = r0[ss], a11 = r0[ss + 1u];
    dst[i] = make_float4(((a00.x + a10.x) + (a01.x + a11.x)) * 0.25f, ((a00.y + a10.y) + (a01.y + a11.y)) * 0.25f,
                         ((a00.z + a10.z) + (a01.z + a11.z)) * 0.25f, ((a00.w + a10.w) + (a01.w + a11.w)) * 0.25f);
}

struct EnvLookupK {
    const float4* in;
    float4* out;
    uint32_t count;
    EnvMapK e;
};

__global__ void __launch_bounds__(256) kenv_lookup(const EnvLookupK k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k.count) return;
    const float4 q = k.in[i];
    float r, g, b;
    const float m = env_color(k.e, q.x, q.y, q.z, q.w, r, g, b);
    k.out[i] = make_float4(r, g, b, m);
}

struct EnvMarchK {
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
    float tau_set;
    EnvMapK e;
};

#define VCT_ENV_ROW(cn, ct, cb, w) {cn, ct, cb, w},
__device__ const float kEnvCones1[1][4] = {VCT_CONES1(VCT_ENV_ROW)};
__device__ const float kEnvCones9[9][4] = {VCT_CONES9(VCT_ENV_ROW)};
__device__ const float kEnvCones16[16][4] = {VCT_CONES16(VCT_ENV_ROW)};
#undef VCT_ENV_ROW

template <bool O32>
__global__ void __launch_bounds__(64) kenv_march(const EnvMarchK k) {
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
    const float(*cones)[4] = k.nd == 16 ? kEnvCones16 : (k.nd == 9 ? kEnvCones9 : kEnvCones1);
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, vis = 0.0f;
    uint32_t steps = 0;
    for (int c = 0; c < k.nd; ++c) {
        const float cn = cones[c][0], ct = cones[c][1], cb = cones[c][2], wk = cones[c][3];
        const float dx = (cn * nx + ct * Tx) + cb * Bx;
        const float dy = (cn * ny + ct * Ty) + cb * By;
        const float dz = (cn * nz + ct * Tz) + cb * Bz;
        const float a = cone<O32>(k, k.tab, valid, ox, oy, oz, dx, dy, dz, __builtin_inff(), steps);
        const float T = fmaxf(1.0f - a / VCT_ALPHA_STOP, 0.0f);
        float sr, sg, sb;
        env_color(k.e, dx, dy, dz, k.tau_set, sr, sg, sb);
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

struct EnvSpecK {
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
    EnvMapK e;
};

// ksky_spec (vct_sky_view.hip), restated: that unit's device code stays as it is
template <bool O32>
__global__ void __launch_bounds__(64) kenv_spec(const EnvSpecK k) {
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
        env_color(k.e, dx, dy, dz, tau, sr, sg, sb);
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

struct EnvBgK {
    const float4* pos;
    float4* lin;
    uint32_t* rgba8;
    uint32_t npx;
    int w, h;
    float fx, fy, fz, ux, uy, uz, rx, ry, rz, tan_half, aspect;   // vct_view.h camera_fields
    EnvMapK e;
};

template <bool LIN, bool RGBA>
__global__ void __launch_bounds__(256) kenv_bg(const EnvBgK k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k.npx) return;
    const float4 P = k.pos[i];
    if (P.w != 0.0f) return;
    const int y = (int)(i / (uint32_t)k.w), x = (int)(i - (uint32_t)y * (uint32_t)k.w);
    float dx, dy, dz, r, g, b;
    pixel_ray(k, x, y, dx, dy, dz);
    env_color(k.e, dx, dy, dz, 0.0f, r, g, b);
    if constexpr (LIN) k.lin[i] = make_float4(r, g, b, 1.0f);
    if constexpr (RGBA) k.rgba8[i] = to8(r) | (to8(g) << 8) | (to8(b) << 16) | (255u << 24);
}

// ---- host side --------------------------------------------------------------------------
std::atomic<int> g_env_force64{0};   // vct_debug_env: every grid takes the 64-bit path

// the input rule of vct_spec.h "environment sky" on a record; nullptr, or what is wrong
const char* check_env_record(const vct_env_sky& in) {
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(in.frame[i][k])) return "non-finite frame";
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            const double g = ((double)in.frame[i][0] * in.frame[j][0] + (double)in.frame[i][1] * in.frame[j][1]) +
                             (double)in.frame[i][2] * in.frame[j][2];
            if (!(fabs(g - (i == j ? 1.0 : 0.0)) <= VCT_GBUF_ORTHO_EPS)) return "frame rows not orthonormal to VCT_GBUF_ORTHO_EPS";
        }
    if (!std::isfinite(in.scale)) return "non-finite scale";
    if (std::signbit(in.scale)) return "negative scale";
    if (in.scale > VCT_ENV_TEXEL_LIMIT) return "scale above VCT_ENV_TEXEL_LIMIT";
    return nullptr;
}

// the record rule, then the map: fills e, or sets the error and returns its status
vct_status prepare_env(vct_ctx* c, const char* what, const vct_env_sky& in, EnvMapK& e) {
    if (const char* bad = check_env_record(in)) return lfail(c, VCT_EINVAL, std::string(what) + ": " + bad);
    const Env& m = c->env;
    if (!m.size || !m.map) return lfail(c, VCT_ESTATE, std::string(what) + " without an environment map (vct_set_env)");
    e.map = m.map;
    e.s2 = m.size * m.size;
    e.lg = (int)m.lg;
    e.Sf = (float)m.size;
    e.lgf = (float)m.lg;
    std::memcpy(e.f, in.frame, sizeof e.f);
    e.scale = in.scale;
    return VCT_OK;
}

// the march over a w x h G-buffer, queued on the ctx stream; k.e is filled (sky_march of vct_sky.hip)
vct_status env_march(vct_ctx* c, const char* what, EnvMarchK& k, const float4* pos, const float4* nrm, uint32_t w,
                     uint32_t h, float4* sky4, float4* diff, unsigned long long* cone_steps) {
    const Grid& g = c->grid;
    hipError_t e;
    const std::string name(what);
    k.nd = (int)c->cfg.n_diffuse;
    k.tau_set = k.nd == 16 ? VCT_TAN20 : VCT_TAN30;
    if (k.nd != 0) {
        // the diffuse aperture's table, from the context's set (ordered after its last march)
        const float tau = k.tau_set;
        uint8_t slot = 0;
        const StepRow* tabs = nullptr;
        if ((e = tables_enter(c)) != hipSuccess) return lhip(c, e, (name + ": stream wait").c_str());
        vct_status st = step_tables(c, what, &tau, 1, &slot, &tabs);
        if (st != VCT_OK) return st;
        k.tab = tabs + (size_t)slot * kShadowRows;
    }
    const bool o32 = g.n <= 512 && !g_env_force64.load();
    alpha_ranges(g, o32, k.lvl);
    k.pos = pos; k.nrm = nrm;
    k.sky = sky4; k.diff = diff; k.steps_total = cone_steps;
    k.n = (int)g.n; k.L = (int)g.L; k.lgn = __builtin_ctz(g.n); k.aniso = g.aniso;
    k.w = (int)w; k.h = (int)h; k.tiles_x = (int)((w + 7) / 8);
    k.g0x = g.g0[0]; k.g0y = g.g0[1]; k.g0z = g.g0[2]; k.inv_h = g.inv_h;
    k.tmax = (float)g.n * VCT_SQRT3;
    const uint32_t blocks = (uint32_t)k.tiles_x * ((h + 7) / 8);
    if (o32) hipLaunchKernelGGL(kenv_march<true>, dim3(blocks), dim3(64), 0, c->stream, k);
    else hipLaunchKernelGGL(kenv_march<false>, dim3(blocks), dim3(64), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, what);
    c->env.path = o32 ? 32 : 64;
    if (k.nd != 0 && (e = tables_leave(c)) != hipSuccess) return lhip(c, e, (name + ": event record").c_str());
    return VCT_OK;
}

}  // namespace

void env_free(vct_ctx* c) {
    if (c->env.map) (void)hipFree(c->env.map);
    c->env.map = nullptr;
    c->env.size = c->env.lg = 0;
}

}  // namespace vct

using namespace vct;

extern "C" vct_status vct_set_env(vct_ctx* c, const float* host_oct4, uint32_t size) {
    if (!c) return VCT_EINVAL;
    hipError_t e;
    if (size == 0) {
        if ((e = hipSetDevice(c->device)) != hipSuccess) return lhip(c, e, "hipSetDevice");
        if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return lhip(c, e, "set_env: stream synchronize");
        env_free(c);
        return VCT_OK;
    }
    if (!host_oct4) return lfail(c, VCT_EINVAL, "set_env: NULL map");
    if (size > VCT_ENV_MAX_DIM || (size & (size - 1u)) != 0u)
        return lfail(c, VCT_EINVAL, "set_env: size must be a power of two in 1..VCT_ENV_MAX_DIM");
    const uint32_t s2 = size * size;
    for (uint32_t t = 0; t < s2; ++t)
        for (int k = 0; k < 3; ++k) {
            const float v = host_oct4[4 * (size_t)t + k];
            if (!std::isfinite(v)) return lfail(c, VCT_EINVAL, "set_env: non-finite texel");
            if (std::signbit(v)) return lfail(c, VCT_EINVAL, "set_env: negative texel");
            if (v > VCT_ENV_TEXEL_LIMIT) return lfail(c, VCT_EINVAL, "set_env: texel above VCT_ENV_TEXEL_LIMIT");
        }
    if ((e = hipSetDevice(c->device)) != hipSuccess) return lhip(c, e, "hipSetDevice");
    const uint32_t lg = (uint32_t)__builtin_ctz(size);
    const size_t texels = (size_t)env_level_off(s2, 1u) + 1u;   // through the one texel of level lg
    float4* map = nullptr;
    if ((e = hipMalloc((void**)&map, texels * sizeof(float4))) != hipSuccess) return lhip(c, e, "set_env: hipMalloc");
    e = hipMemcpyAsync(map, host_oct4, (size_t)s2 * sizeof(float4), hipMemcpyHostToDevice, c->stream);
    hipEvent_t ev[2] = {nullptr, nullptr};                  // vct_debug_env_mips: around the mip kernels
    const bool timed = c->env.profile && e == hipSuccess && hipEventCreate(&ev[0]) == hipSuccess &&
                       hipEventCreate(&ev[1]) == hipSuccess && hipEventRecord(ev[0], c->stream) == hipSuccess;
    for (uint32_t j = 0; e == hipSuccess && j < lg; ++j) {
        const uint32_t sd = size >> (j + 1u);
        hipLaunchKernelGGL(kenv_mip, dim3((sd * sd + 255u) / 256u), dim3(256), 0, c->stream,
                           map + env_level_off(s2, size >> j), map + env_level_off(s2, sd), sd);
        e = hipGetLastError();
    }
    if (timed && e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
    // the upload has left host_oct4, and every earlier call on the stream the previous map
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (timed && e == hipSuccess) e = hipEventElapsedTime(&c->env.mip_ms, ev[0], ev[1]);
    for (hipEvent_t v : ev)
        if (v) (void)hipEventDestroy(v);
    if (e != hipSuccess) {
        (void)hipFree(map);
        return lhip(c, e, "set_env: upload / mip build");
    }
    env_free(c);
    c->env.map = map;
    c->env.size = size;
    c->env.lg = lg;
    return VCT_OK;
}

extern "C" uint32_t vct_env_size(const vct_ctx* c) { return c ? c->env.size : 0u; }

extern "C" vct_status vct_env_download_level(vct_ctx* c, uint32_t level, float* host_rgba) {
    if (!c) return VCT_EINVAL;
    if (!host_rgba) return lfail(c, VCT_EINVAL, "env_download_level: NULL buffer");
    const Env& m = c->env;
    if (!m.size) return lfail(c, VCT_ESTATE, "env_download_level without an environment map (vct_set_env)");
    if (level > m.lg) return lfail(c, VCT_EINVAL, "env_download_level: level above lg size");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    const uint32_t sj = m.size >> level;
    e = hipMemcpy(host_rgba, m.map + env_level_off(m.size * m.size, sj), (size_t)sj * sj * sizeof(float4),
                  hipMemcpyDeviceToHost);
    if (e != hipSuccess) return lhip(c, e, "env_download_level: copy");
    return VCT_OK;
}

extern "C" vct_status vct_env_lookup_device(vct_ctx* c, const vct_env_sky* env, const float* dir_tau4, uint32_t count,
                                            float* out4) {
    if (!c) return VCT_EINVAL;
    if (!env) return lfail(c, VCT_EINVAL, "env_lookup: NULL env");
    if (count > 0x7fffffffu) return lfail(c, VCT_EINVAL, "env_lookup: count too large");
    if (count != 0 && (!dir_tau4 || !out4)) return lfail(c, VCT_EINVAL, "env_lookup: NULL buffer");
    if ((((uintptr_t)dir_tau4 | (uintptr_t)out4) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "env_lookup: float4 buffers must be 16-byte aligned");
    EnvLookupK k;
    std::memset(&k, 0, sizeof k);
    vct_status st = prepare_env(c, "env_lookup", *env, k.e);
    if (st != VCT_OK) return st;
    if (count == 0) return VCT_OK;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    k.in = (const float4*)dir_tau4; k.out = (float4*)out4; k.count = count;
    hipLaunchKernelGGL(kenv_lookup, dim3((count + 255u) / 256u), dim3(256), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "env_lookup");
    return VCT_OK;
}

extern "C" vct_status vct_env_cones_device(vct_ctx* c, const float* pos4, const float* nrm4, uint32_t w, uint32_t h,
                                           const vct_env_sky* env, float* sky4, float* diffuse4_inout,
                                           unsigned long long* cone_steps) {
    if (!c) return VCT_EINVAL;
    if (!pos4 || !nrm4 || !sky4 || w == 0 || h == 0) return lfail(c, VCT_EINVAL, "env_cones: NULL buffer or empty frame");
    if (!env) return lfail(c, VCT_EINVAL, "env_cones: NULL env");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "env_cones: frame too large");
    if ((((uintptr_t)pos4 | (uintptr_t)nrm4 | (uintptr_t)sky4 | (uintptr_t)diffuse4_inout) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "env_cones: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)cone_steps & 7u) != 0) return lfail(c, VCT_EINVAL, "env_cones: cone_steps must be 8-byte aligned");
    EnvMarchK k;
    std::memset(&k, 0, sizeof k);
    vct_status st = prepare_env(c, "env_cones", *env, k.e);
    if (st != VCT_OK) return st;
    const Grid& g = c->grid;
    if (!g.voxelized || !g.mipped) return lfail(c, VCT_ESTATE, "env_cones before voxelize / build_mips");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    return env_march(c, "env_cones", k, (const float4*)pos4, (const float4*)nrm4, w, h, (float4*)sky4,
                     (float4*)diffuse4_inout, cone_steps);
}

extern "C" vct_status vct_inject_env(vct_ctx* c, const vct_env_sky* env) {
    if (!c) return VCT_EINVAL;
    if (!env) return lfail(c, VCT_EINVAL, "inject_env: NULL env");
    EnvMarchK k;
    std::memset(&k, 0, sizeof k);
    vct_status st = prepare_env(c, "inject_env", *env, k.e);
    if (st != VCT_OK) return st;
    Grid& g = c->grid;
    if (!g.voxelized) return lfail(c, VCT_ESTATE, "inject_env before voxelize");
    if (!g.injected || !g.mipped) return lfail(c, VCT_ESTATE, "inject_env before inject / build_mips");
    if (g.skied)
        return lfail(c, VCT_ESTATE, "inject_env after inject_sky / inject_env on this level 0 (inject or upload a new one first)");
    if (g.bounced)
        return lfail(c, VCT_ESTATE, "inject_env after inject_bounces on this level 0 (the bounce's level 0 must "
                                    "already hold the sky)");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    if ((e = bounce_sources(c)) != hipSuccess) return lhip(c, e, "inject_env: bounce sources");
    g.skied = true;
    const Bounce& b = c->bounce;
    // no cone (Sk = 0) or no source: level 0 and its mips stay as they are
    if (c->cfg.n_diffuse == 0 || b.n_src == 0) return VCT_OK;
    // Sk into the specular plane of the source G-buffer, as vct_inject_sky does
    constexpr int kPlane = 3;
    st = env_march(c, "inject_env", k, b.gbuf, b.gbuf + b.px_cap, b.tiles_x * VCT_TILE, b.tiles_y * VCT_TILE,
                   b.gbuf + (size_t)kPlane * b.px_cap, nullptr, nullptr);
    if (st != VCT_OK) return st;
    if ((e = launch_bounce_add_plane(c, kPlane)) != hipSuccess) return lhip(c, e, "inject_env: add");
    g.mipped = false;
    g.l0_on_peers = false;   // device 0 added: vct_build_mips copies level 0 to the other devices
    // a relight build: level 0 is still nonzero exactly at the occupied voxels (alpha untouched)
    return vct_build_mips(c);
}

extern "C" vct_status vct_env_specular_device(vct_ctx* c, const float* pos4, const float* nrm4, const float* alb4,
                                              uint32_t w, uint32_t h, const float* eye, const vct_env_sky* env,
                                              float* skyspec4, float* spec4_inout, unsigned long long* cone_steps) {
    if (!c) return VCT_EINVAL;
    if (!pos4 || !nrm4 || !alb4 || !skyspec4 || !eye || w == 0 || h == 0)
        return lfail(c, VCT_EINVAL, "env_specular: NULL buffer or empty frame");
    if (!env) return lfail(c, VCT_EINVAL, "env_specular: NULL env");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "env_specular: frame too large");
    if ((((uintptr_t)pos4 | (uintptr_t)nrm4 | (uintptr_t)alb4 | (uintptr_t)skyspec4 | (uintptr_t)spec4_inout) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "env_specular: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)cone_steps & 7u) != 0) return lfail(c, VCT_EINVAL, "env_specular: cone_steps must be 8-byte aligned");
    EnvSpecK k;
    std::memset(&k, 0, sizeof k);
    vct_status st = prepare_env(c, "env_specular", *env, k.e);
    if (st != VCT_OK) return st;
    const Grid& g = c->grid;
    if (!g.voxelized || !g.mipped) return lfail(c, VCT_ESTATE, "env_specular before voxelize / build_mips");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    const bool o32 = g.n <= 512 && !g_env_force64.load();
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
    if (o32) hipLaunchKernelGGL(kenv_spec<true>, dim3(blocks), dim3(64), 0, c->stream, k);
    else hipLaunchKernelGGL(kenv_spec<false>, dim3(blocks), dim3(64), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "env_specular");
    c->env.path = o32 ? 32 : 64;
    return VCT_OK;
}

extern "C" vct_status vct_env_background_device(vct_ctx* c, const vct_camera* cam, const float* pos4, uint32_t w,
                                                uint32_t h, const vct_env_sky* env, float* linear4_inout,
                                                uint32_t* rgba8_inout) {
    if (!c) return VCT_EINVAL;
    if (!cam || !pos4 || w == 0 || h == 0) return lfail(c, VCT_EINVAL, "env_background: NULL camera, NULL buffer or empty frame");
    if (!env) return lfail(c, VCT_EINVAL, "env_background: NULL env");
    if (!linear4_inout && !rgba8_inout) return lfail(c, VCT_EINVAL, "env_background: no output");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "env_background: frame too large");
    if ((((uintptr_t)pos4 | (uintptr_t)linear4_inout) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "env_background: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)rgba8_inout & 3u) != 0) return lfail(c, VCT_EINVAL, "env_background: rgba8 buffer must be 4-byte aligned");
    EnvBgK k;
    std::memset(&k, 0, sizeof k);
    vct_status st = prepare_env(c, "env_background", *env, k.e);
    if (st != VCT_OK) return st;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    camera_fields(k, cam, w, h);
    k.pos = (const float4*)pos4; k.lin = (float4*)linear4_inout; k.rgba8 = rgba8_inout; k.npx = w * h;
    const dim3 grid((k.npx + 255) / 256), block(256);
    if (k.lin && k.rgba8) hipLaunchKernelGGL((kenv_bg<true, true>), grid, block, 0, c->stream, k);
    else if (k.lin) hipLaunchKernelGGL((kenv_bg<true, false>), grid, block, 0, c->stream, k);
    else hipLaunchKernelGGL((kenv_bg<false, true>), grid, block, 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "env_background");
    return VCT_OK;
}

// Test and tool hook (not part of the public headers).  force64 >= 0: nonzero sends every
// grid's env marches through the 64-bit-address path that 1024^3 takes (process-wide).
extern "C" int vct_debug_env(int force64) {
    if (force64 >= 0) g_env_force64.store(force64 ? 1 : 0);
    return 0;
}

// Tool hook.  profile >= 0: nonzero times the mip kernels of the context's following vct_set_env
// calls with events.  Returns the time of the last timed build in ms (0 before the first).
extern "C" float vct_debug_env_mips(vct_ctx* c, int profile) {
    if (!c) return -1.0f;
    if (profile >= 0) c->env.profile = profile != 0;
    return c->env.mip_ms;
}

// The address path the context's last env march (diffuse or specular) was launched with: 32
// (buffer resources), 64 (64-bit addresses), 0 before the first one.
extern "C" int vct_debug_env_path(const vct_ctx* c) { return c ? c->env.path : -1; }
