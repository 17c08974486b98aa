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
//
// The four sky calls are vct_sky_march.h's kernels, launchers and bodies with the map as the
// colour source (EnvMapK::color is env_color), so the marches are the gradient sky's own
// (vct_sky.hip); the only addresses this unit adds are env_color's.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstring>
#include "vct_internal.h"
#include "vct_light_terms.h"
#include "vct_sky_march.h"

namespace vct {
namespace {

static_assert(sizeof(vct_env_sky) == 40, "vct_env_sky is 10 floats (include/vct_env.h)");

// the map and the record, as every kernel here takes them: vct_sky_march.h's colour source
struct EnvMapK {
    const float4* map;
    uint32_t s2;                 // S * S
    int lg;                      // lg S
    float Sf, lgf;               // (float)S, (float)lg S
    float f[3][3];
    float scale;

    __device__ void color(float dx, float dy, float dz, float tau, float& r, float& g, float& b) const;   // env_color
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

__device__ __forceinline__ void EnvMapK::color(float dx, float dy, float dz, float tau, float& r, float& g, float& b) const {
    env_color(*this, dx, dy, dz, tau, r, g, b);
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
    return cones_call<EnvMapK>(c, "env_cones", "env", env, prepare_env, g_env_force64, &c->env.path, pos4, nrm4, w, h, sky4,
                               diffuse4_inout, cone_steps);
}

extern "C" vct_status vct_inject_env(vct_ctx* c, const vct_env_sky* env) {
    if (!c) return VCT_EINVAL;
    return inject_call<EnvMapK>(c, "inject_env", "env", env, prepare_env, g_env_force64, &c->env.path,
                                "inject_env after inject_sky / inject_env on this level 0 (inject or upload a new one first)",
                                false);
}

extern "C" vct_status vct_env_specular_device(vct_ctx* c, const float* pos4, const float* nrm4, const float* alb4,
                                              uint32_t w, uint32_t h, const float* eye, const vct_env_sky* env,
                                              float* skyspec4, float* spec4_inout, unsigned long long* cone_steps) {
    if (!c) return VCT_EINVAL;
    return specular_call<EnvMapK>(c, "env_specular", "env", env, prepare_env, g_env_force64, &c->env.path, pos4, nrm4, alb4,
                                  w, h, eye, skyspec4, spec4_inout, cone_steps);
}

extern "C" vct_status vct_env_background_device(vct_ctx* c, const vct_camera* cam, const float* pos4, uint32_t w,
                                                uint32_t h, const vct_env_sky* env, float* linear4_inout,
                                                uint32_t* rgba8_inout) {
    if (!c) return VCT_EINVAL;
    return background_call<EnvMapK>(c, "env_background", "env", env, prepare_env, cam, pos4, w, h, linear4_inout,
                                    rgba8_inout);
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
