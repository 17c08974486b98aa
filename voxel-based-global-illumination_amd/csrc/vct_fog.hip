// vct_fog.hip — volumetric fog (include/vct_fog.h; the arithmetic is include/vct_spec.h
// "volumetric fog"): a scatter volume built from the radiance pyramid, the view-ray segments
// of a frame, the march that integrates the volume along them, and the line of the composite
// that puts the result on the frame.
//
//   kfog_records  the synthetic G-buffer of the ambient term: 2 m^3 records at the cell
//                 centres, normal +y then -y, which K4 traces through the existing launch
//                 path in a forced form (launch_trace's bounce_form: diffuse cones only, no
//                 tuner), as the bounce gather does.
//   kfog_build    one wave per 4x4x4 block of cells, one lane per cell, the lights in a
//                 wave-uniform loop (ks_march's shape): a light no lane needs is skipped on a
//                 ballot, every other one marches vct_alpha_march.h's lockstep cone from the
//                 cell centre.  The lane then combines its sum with the ambient planes and
//                 writes S into the volume, so there is no separate combine launch.
//   kfog_rays     one lane per pixel: (d, len) of the eye -> pixel segment, or the caster's
//                 primary ray (vct_view.h pixel_ray) for a background pixel.
//   kfog_march    the hot kernel: one wave per 8x8 pixel block, one lane per pixel.  The
//                 volume is in the pyramid's brick layout (eight float4 cells of a 2x2x2
//                 block per 128 bytes) and is read through a buffer resource with 16-byte
//                 loads: the edge clamp is integer min / max on the corner indices before the
//                 address is formed, an ended lane's x field is replaced by one past any
//                 volume, so the hardware range check answers +0 and nothing is selected
//                 behind a load.  An ended lane composites with a = 0, which changes neither
//                 F nor T; the wave ends on a bare-compare ballot.
//   kfog_apply    rgb = fmaf(rgb, T, F) and the tone curve (vct_view.h to8).
//
// The volume is at most 512^3 cells (n = 1024, level 1): 2^31 bytes, inside a buffer
// resource's 32-bit range, so the march has one address path for every grid.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>
#include "vct_internal.h"
#include "vct_light_terms.h"
#include "vct_alpha_march.h"
#include "vct_view.h"

namespace vct {
namespace {

static_assert(sizeof(vct_fog) == 28, "vct_fog is 7 dwords (include/vct_fog.h)");

// ---- the scatter volume -------------------------------------------------------------------
struct FogBuildK {
    float4* vol;                 // m^3 cells, brick layout
    const float4* amb;           // [2][m^3] K4's diffuse plane of the +y / -y records, or null
    const StepRow* tabs;         // [slot][kShadowRows]
    unsigned long long* steps_total;
    AlphaRange lvl[kMaxLevels + 1];
    int n, L, lgn, aniso;
    int m, lgm;
    uint32_t n_lights;
    float tmax, h2, cs;
    float ar, ag, ab, ambient;
    uint8_t slot[VCT_MAX_LIGHTS];
};

struct FogRecK {
    float4* pos;
    float4* nrm;
    uint32_t cells;              // m^3
    int m, lgm;
    float g0x, g0y, g0z, hh, cs;
};

__global__ void __launch_bounds__(256) kfog_records(const FogRecK k) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= 2u * k.cells) return;
    const uint32_t v = r < k.cells ? r : r - k.cells;
    const uint32_t mask = (uint32_t)k.m - 1u;
    const uint32_t i = v & mask, j = (v >> k.lgm) & mask, l = v >> (2 * k.lgm);
    const float xc = ((float)i + 0.5f) * k.cs, yc = ((float)j + 0.5f) * k.cs, zc = ((float)l + 0.5f) * k.cs;
    k.pos[r] = make_float4(k.g0x + xc * k.hh, k.g0y + yc * k.hh, k.g0z + zc * k.hh, 1.0f);
    k.nrm[r] = make_float4(0.0f, r < k.cells ? 1.0f : -1.0f, 0.0f, 0.0f);
}

// "volumetric fog": a light's direction, factor and distance at a cell centre; false: skipped
__device__ __forceinline__ bool fog_terms(const DLight& L, float h2, float qx, float qy, float qz, float& lx, float& ly,
                                          float& lz, float& att, float& t_lim) {
    if (L.type == VCT_LIGHT_DIRECTIONAL) {
        lx = L.ax; ly = L.ay; lz = L.az;
        att = 1.0f;
        t_lim = __builtin_inff();
        return true;
    }
    const float dx = L.px - qx, dy = L.py - qy, dz = L.pz - qz;
    const float r2 = dot3(dx, dy, dz, dx, dy, dz);
    if (!(r2 > 0.0f)) return false;
    const float r = sqrtf(r2);
    lx = dx / r; ly = dy / r; lz = dz / r;
    t_lim = r;
    const float u = r2 * L.inv_rr;
    const float w = fmaxf(1.0f - u, 0.0f);
    att = (w * w) / (1.0f + r2 * h2);
    if (L.type == VCT_LIGHT_SPOT) {
        const float cd = dot3(lx, ly, lz, L.ax, L.ay, L.az);
        const float s = fminf(fmaxf((cd - L.cos_outer) * L.inv_span, 0.0f), 1.0f);
        att = att * (s * s);
    }
    return att > 0.0f;
}

template <bool O32>
__global__ void __launch_bounds__(64) kfog_build(const FogBuildK k, const LightSet set) {
    const int lane = (int)threadIdx.x;
    const uint32_t lgb = (uint32_t)k.lgm - 2u, mb = 1u << lgb;          // 4x4x4 blocks per axis
    const uint32_t b = blockIdx.x;
    const uint32_t i = ((b & (mb - 1u)) << 2) | (uint32_t)(lane & 3);
    const uint32_t j = (((b >> lgb) & (mb - 1u)) << 2) | (uint32_t)((lane >> 2) & 3);
    const uint32_t l = ((b >> (2u * lgb)) << 2) | (uint32_t)(lane >> 4);
    const float xc = ((float)i + 0.5f) * k.cs, yc = ((float)j + 0.5f) * k.cs, zc = ((float)l + 0.5f) * k.cs;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
    uint32_t steps = 0;
    for (uint32_t q = 0; q < k.n_lights; ++q) {
        const DLight& L = set.l[q];
        float lx = 0.0f, ly = 0.0f, lz = 0.0f, att = 0.0f, t_lim = 0.0f;
        const bool need = fog_terms(L, k.h2, xc, yc, zc, lx, ly, lz, att, t_lim);
        if (__builtin_amdgcn_ballot_w64(need) == 0ull) continue;
        const StepRow* tab = k.tabs + (size_t)k.slot[q] * kShadowRows;
        float a;
        if (L.type == VCT_LIGHT_DIRECTIONAL)   // l is the light's: faces and d^2 are scalar
            a = cone<O32>(k, tab, need, xc, yc, zc, L.ax, L.ay, L.az, __builtin_inff(), steps);
        else
            a = cone<O32>(k, tab, need, xc, yc, zc, lx, ly, lz, t_lim, steps);
        const float V = fmaxf(1.0f - a / VCT_ALPHA_STOP, 0.0f);
        const float w = att * V;
        if (need) {
            ar = fmaf(L.cr, w, ar);
            ag = fmaf(L.cg, w, ag);
            ab = fmaf(L.cb, w, ab);
        }
    }
    float sr = VCT_FOG_PHASE * ar, sg = VCT_FOG_PHASE * ag, sb = VCT_FOG_PHASE * ab;
    if (k.ambient > 0.0f) {
        float Ar = 0.0f, Ag = 0.0f, Ab = 0.0f;
        if (k.amb) {
            const uint32_t v = i | (j << k.lgm) | (l << (2 * k.lgm));
            const float4 Ip = k.amb[v], Im = k.amb[(size_t)v + ((size_t)1 << (3 * k.lgm))];
            Ar = 0.5f * (Ip.x + Im.x);
            Ag = 0.5f * (Ip.y + Im.y);
            Ab = 0.5f * (Ip.z + Im.z);
        }
        sr = fmaf(k.ambient, Ar, sr);
        sg = fmaf(k.ambient, Ag, sg);
        sb = fmaf(k.ambient, Ab, sb);
    }
    k.vol[texel_index_lg(i, j, l, (uint32_t)k.lgm)] = make_float4(k.ar * sr, k.ag * sg, k.ab * sb, 0.0f);
    if (k.steps_total) {
        const uint32_t ws = wave_sum_u32(steps);
        if (lane == 0 && ws) atomicAdd(k.steps_total, (unsigned long long)ws);
    }
}

// ---- the segments ---------------------------------------------------------------------------
struct FogRayK {
    const float4* pos;
    float4* ray;
    int w, h;
    int has_cam;
    float fx, fy, fz, ux, uy, uz, rx, ry, rz, tan_half, aspect;
    float ox, oy, oz;            // the eye in voxel units
    float g0x, g0y, g0z, inv_h;
};

__device__ __forceinline__ bool finitef(float v) { return fabsf(v) < __builtin_inff(); }

__global__ void __launch_bounds__(256) kfog_rays(const FogRayK k) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (uint32_t)k.w * (uint32_t)k.h) return;
    const float4 P = k.pos[p];
    float dx = 0.0f, dy = 0.0f, dz = 0.0f, len = 0.0f;
    bool ok;
    if (P.w != 0.0f) {
        const float ex = (P.x - k.g0x) * k.inv_h, ey = (P.y - k.g0y) * k.inv_h, ez = (P.z - k.g0z) * k.inv_h;
        const float vx = ex - k.ox, vy = ey - k.oy, vz = ez - k.oz;
        len = sqrtf((vx * vx + vy * vy) + vz * vz);
        dx = vx / len; dy = vy / len; dz = vz / len;
        ok = len > 0.0f && finitef(len);
    } else if (k.has_cam) {
        const int y = (int)(p / (uint32_t)k.w), x = (int)(p - (uint32_t)y * (uint32_t)k.w);
        pixel_ray(k, x, y, dx, dy, dz);
        len = __builtin_inff();
        ok = true;
    } else {
        ok = false;
    }
    ok = ok && finitef(dx) && finitef(dy) && finitef(dz);
    k.ray[p] = ok ? make_float4(dx, dy, dz, len) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ---- the march ------------------------------------------------------------------------------
struct FogMarchK {
    const float4* ray;
    float4* out;
    unsigned long long* steps_total;
    const float4* vol;
    uint32_t vol_bytes;
    int w, h, tiles_x;
    int m, lgm;
    float nf, ox, oy, oz;
    float sigma, ds, inv_cs;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// one axis of the slab test: narrows [t0, t1]; false: the axis empties the segment
__device__ __forceinline__ bool slab_axis(float o, float d, float nf, float& t0, float& t1) {
    const float inv = 1.0f / d;
    if (d == 0.0f || !finitef(inv)) return o >= 0.0f && o <= nf;
    const float ta = (0.0f - o) * inv, tb = (nf - o) * inv;
    t0 = fmaxf(t0, fminf(ta, tb));
    t1 = fminf(t1, fmaxf(ta, tb));
    return true;
}

__global__ void __launch_bounds__(64) kfog_march(const FogMarchK k) {
    const int lane = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / k.tiles_x, tx = (int)blockIdx.x - ty * k.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const bool inframe = x < k.w && y < k.h;
    const size_t px = inframe ? (size_t)y * (size_t)k.w + (size_t)x : 0u;
    const float4 R = k.ray[px];
    bool ok = inframe && R.w > 0.0f && finitef(R.x) && finitef(R.y) && finitef(R.z);
    // a lane without a segment marches a zero ray from the origin: every value it computes is finite
    const float dx = ok ? R.x : 0.0f, dy = ok ? R.y : 0.0f, dz = ok ? R.z : 0.0f;
    float t0 = 0.0f, t1 = ok ? R.w : 0.0f;
    ok = ok & slab_axis(k.ox, dx, k.nf, t0, t1);
    ok = ok & slab_axis(k.oy, dy, k.nf, t0, t1);
    ok = ok & slab_axis(k.oz, dz, k.nf, t0, t1);
    ok = ok && t1 > t0;
    if (!ok) { t0 = 0.0f; t1 = 0.0f; }
    const float span = t1 - t0;
    const int N = ok ? (int)fminf(ceilf(span / k.ds), (float)VCT_FOG_MAX_STEPS) : 0;
    const float a_full = fminf(k.sigma * k.ds, 1.0f);
    const float a_last = fminf(k.sigma * fminf(span - (float)(N - 1) * k.ds, k.ds), 1.0f);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)k.vol, (short)0, (int)k.vol_bytes, 0x00020000);
    const int hi = k.m - 1;
    const uint32_t lnb = (uint32_t)k.lgm - 1u;
    float T = 1.0f, Fr = 0.0f, Fg = 0.0f, Fb = 0.0f;
    uint32_t cnt = 0;
    for (int i = 0; i < VCT_FOG_MAX_STEPS; ++i) {
        const bool act = (i < N) & !(T < VCT_FOG_T_STOP);
        if (__builtin_amdgcn_ballot_w64(act) == 0ull) break;
        const float ts = t0 + ((float)i + 0.5f) * k.ds;
        const float cx = (k.ox + dx * ts) * k.inv_cs - 0.5f, cy = (k.oy + dy * ts) * k.inv_cs - 0.5f,
                    cz = (k.oz + dz * ts) * k.inv_cs - 0.5f;
        const float flx = floorf(cx), fly = floorf(cy), flz = floorf(cz);
        const float wx1 = cx - flx, wy1 = cy - fly, wz1 = cz - flz;
        const float wx[2] = {1.0f - wx1, wx1}, wy[2] = {1.0f - wy1, wy1}, wz[2] = {1.0f - wz1, wz1};
        // the float -> int conversion saturates; the clamp brings every index into [0, m - 1]
        const int ix = (int)fminf(fmaxf(flx, -1.0f), (float)k.m), iy = (int)fminf(fmaxf(fly, -1.0f), (float)k.m),
                  iz = (int)fminf(fmaxf(flz, -1.0f), (float)k.m);
        uint32_t xs[2], ys[2], zs[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint32_t ux = (uint32_t)min(max(ix + c, 0), hi), uy = (uint32_t)min(max(iy + c, 0), hi),
                           uz = (uint32_t)min(max(iz + c, 0), hi);
            xs[c] = act ? (((ux >> 1) << 3) | (ux & 1u)) : kOutT;
            ys[c] = ((uy >> 1) << (lnb + 3u)) | ((uy & 1u) << 1);
            zs[c] = ((uz >> 1) << (2u * lnb + 3u)) | ((uz & 1u) << 2);
        }
        u32x4 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c)
            v[c] = __builtin_amdgcn_raw_buffer_load_b128(rs, (xs[c & 1] | ys[(c >> 1) & 1] | zs[c >> 2]) << 4, 0, 0);
        float Sr = 0.0f, Sg = 0.0f, Sb = 0.0f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float wc = (wx[c & 1] * wy[(c >> 1) & 1]) * wz[c >> 2];
            Sr = fmaf(wc, __uint_as_float(v[c].x), Sr);
            Sg = fmaf(wc, __uint_as_float(v[c].y), Sg);
            Sb = fmaf(wc, __uint_as_float(v[c].z), Sb);
        }
        const float a = act ? (i == N - 1 ? a_last : a_full) : 0.0f;
        const float Ta = T * a;
        Fr = fmaf(Ta, Sr, Fr);
        Fg = fmaf(Ta, Sg, Fg);
        Fb = fmaf(Ta, Sb, Fb);
        T = T * (1.0f - a);
        cnt += act ? 1u : 0u;
    }
    if (inframe) k.out[px] = make_float4(Fr, Fg, Fb, T);
    if (k.steps_total) {
        const uint32_t ws = wave_sum_u32(cnt);
        if (lane == 0 && ws) atomicAdd(k.steps_total, (unsigned long long)ws);
    }
}

// ---- apply ------------------------------------------------------------------------------------
struct FogApplyK {
    const float4* fog;
    float4* lin;
    uint32_t* rgba8;
    uint32_t npx;
};

__global__ void __launch_bounds__(256) kfog_apply(const FogApplyK k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k.npx) return;
    const float4 G = k.fog[i];
    const float4 B = k.lin ? k.lin[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 C = make_float4(fmaf(B.x, G.w, G.x), fmaf(B.y, G.w, G.y), fmaf(B.z, G.w, G.z), B.w);
    if (k.lin) k.lin[i] = C;
    if (!k.rgba8) return;
    if (B.w == 0.0f) {
        // a background pixel: the composite presents its clear colour as it is, without the tone
        // curve, so the fog goes over it in display space -- with T = 1 and F = 0 the byte is the
        // composite's
        k.rgba8[i] = quant8(fmaf(B.x, G.w, tone01(G.x))) | (quant8(fmaf(B.y, G.w, tone01(G.y))) << 8) |
                     (quant8(fmaf(B.z, G.w, tone01(G.z))) << 16) | (255u << 24);
        return;
    }
    k.rgba8[i] = to8(C.x) | (to8(C.y) << 8) | (to8(C.z) << 16) | (255u << 24);
}

// ---- host side --------------------------------------------------------------------------------
std::atomic<int> g_fog_force64{0};   // vct_debug_fog: the light cones of every grid take the 64-bit path

// the input rule of vct_spec.h "volumetric fog"; fills sigma_v, or returns what is wrong
const char* check_fog(const Grid& g, const vct_fog& f, float& sigma) {
    if (!std::isfinite(f.density) || std::signbit(f.density)) return "density must be finite with a clear sign bit";
    if (f.density > VCT_FOG_DENSITY_LIMIT) return "density above VCT_FOG_DENSITY_LIMIT";
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(f.albedo[k]) || std::signbit(f.albedo[k]) || f.albedo[k] > 1.0f)
            return "albedo must be finite and in [0, 1] (-0.0f is refused)";
    if (!std::isfinite(f.ambient) || !(f.ambient >= 0.0f)) return "ambient must be finite and >= 0";
    if (f.level < 1u || f.level > 31u || (g.n >> f.level) < 4u) return "level must satisfy 1 <= level and (n >> level) >= 4";
    if (!(f.step >= 0.25f && f.step <= 4.0f)) return "step must be in [0.25, 4]";
    sigma = (f.density * g.extent) / (float)g.n;
    if (!std::isfinite(sigma)) return "density * extent overflows";
    return nullptr;
}

// o = (eye - g0) * inv_h; false: eye or o is not finite
bool fog_origin(const Grid& g, const float* eye, float* o) {
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(eye[k])) return false;
        o[k] = (eye[k] - g.g0[k]) * g.inv_h;
        if (!std::isfinite(o[k])) return false;
    }
    return true;
}

float exp2_level(uint32_t level) { return (float)(1u << level); }

}  // namespace

void fog_free(vct_ctx* c) {
    Fog& f = c->fog;
    if (f.vol) (void)hipFree(f.vol);
    if (f.gbuf) (void)hipFree(f.gbuf);
    f = Fog{};
}

}  // namespace vct

using namespace vct;

extern "C" vct_status vct_build_fog(vct_ctx* c, const vct_fog* fog, const vct_light* lights, uint32_t n_lights,
                                    const float* tan_half) {
    if (!c) return VCT_EINVAL;
    if (!fog) return lfail(c, VCT_EINVAL, "build_fog: NULL fog");
    if (n_lights > VCT_MAX_LIGHTS) return lfail(c, VCT_EINVAL, "build_fog: more than VCT_MAX_LIGHTS lights");
    if (n_lights && !tan_half) return lfail(c, VCT_EINVAL, "build_fog: NULL tan_half");
    for (uint32_t j = 0; j < n_lights; ++j)
        if (!std::isfinite(tan_half[j]) || !(tan_half[j] > 0.0f))
            return lfail(c, VCT_EINVAL, "build_fog: tan_half[" + std::to_string(j) + "] must be finite and > 0");
    Grid& g = c->grid;
    float sigma = 0.0f;
    if (const char* bad = check_fog(g, *fog, sigma)) return lfail(c, VCT_EINVAL, std::string("build_fog: ") + bad);
    LightSet set;
    std::memset(&set, 0, sizeof set);
    vct_status st = prepare_list(c, "build_fog", lights, n_lights, set.l);
    if (st != VCT_OK) return st;
    if (!g.voxelized || !g.mipped) return lfail(c, VCT_ESTATE, "build_fog before voxelize / build_mips");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");

    Fog& f = c->fog;
    const uint32_t m = g.n >> fog->level;
    const size_t cells = (size_t)m * m * m;
    const int lgm = __builtin_ctz(m);
    if (f.cap < cells) {                       // the first build, or a finer one (hipFree waits for the device)
        if (f.vol) (void)hipFree(f.vol);
        f.vol = nullptr; f.cap = 0; f.built = false;
        if ((e = hipMalloc((void**)&f.vol, cells * sizeof(float4))) != hipSuccess) return lhip(c, e, "build_fog: volume");
        f.cap = cells;
    }
    f.built = false;                           // from here on the volume is rewritten
    const float cs = exp2_level(fog->level);
    const bool ambient = fog->ambient > 0.0f && c->cfg.n_diffuse != 0;
    if (ambient) {
        if (f.gbuf_cap < 2 * cells) {
            if (f.gbuf) (void)hipFree(f.gbuf);
            f.gbuf = nullptr; f.gbuf_cap = 0;
            if ((e = hipMalloc((void**)&f.gbuf, 4 * 2 * cells * sizeof(float4))) != hipSuccess)
                return lhip(c, e, "build_fog: ambient records");
            f.gbuf_cap = 2 * cells;
        }
        FogRecK r;
        r.pos = f.gbuf; r.nrm = f.gbuf + f.gbuf_cap;
        r.cells = (uint32_t)cells; r.m = (int)m; r.lgm = lgm;
        r.g0x = g.g0[0]; r.g0y = g.g0[1]; r.g0z = g.g0[2];
        r.hh = g.extent / (float)g.n; r.cs = cs;
        hipLaunchKernelGGL(kfog_records, dim3((uint32_t)((2 * cells + 255) / 256)), dim3(256), 0, c->stream, r);
        if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "build_fog: ambient records");
        vct_trace_args a{};
        a.pos4 = (const float*)f.gbuf;
        a.nrm4 = (const float*)(f.gbuf + f.gbuf_cap);
        a.alb4 = a.nrm4;                       // roughness belongs to the specular cone: never read
        a.diffuse4 = (float*)(f.gbuf + 2 * f.gbuf_cap);
        a.spec4 = (float*)(f.gbuf + 3 * f.gbuf_cap);
        a.width = m;                           // 2 m^2 rows of m records: row-major = the cells' linear order
        a.height = 2u * m * m;
        a.cone_steps = f.dbg_ambient_steps;
        if ((e = launch_trace(c, &a, c->bounce.form)) != hipSuccess) return lhip(c, e, "build_fog: ambient gather");
    }
    FogBuildK k;
    std::memset(&k, 0, sizeof k);
    if ((e = tables_enter(c)) != hipSuccess) return lhip(c, e, "build_fog: stream wait");
    // As in vct_shadow_cones_device, a failure of step_tables returns without tables_leave, here
    // with the volume already marked as not built and the ambient gather queued.  Its one
    // VCT_EINVAL (an aperture that needs more than kShadowRows rows) cannot happen: the clamp to
    // VCT_SPEC_TAU_MIN needs 265 rows on 1024^3, so what is left are device errors, after which
    // "nothing changed" is not promised.
    if (n_lights && (st = step_tables(c, "build_fog", tan_half, n_lights, k.slot, &k.tabs)) != VCT_OK) return st;
    const bool o32 = g.n <= 512 && !g_fog_force64.load();
    alpha_ranges(g, o32, k.lvl);
    k.vol = f.vol;
    k.amb = ambient ? f.gbuf + 2 * f.gbuf_cap : nullptr;
    k.steps_total = f.dbg_light_steps;
    k.n = (int)g.n; k.L = (int)g.L; k.lgn = __builtin_ctz(g.n); k.aniso = g.aniso;
    k.m = (int)m; k.lgm = lgm;
    k.n_lights = n_lights;
    k.tmax = (float)g.n * VCT_SQRT3; k.h2 = grid_h2(g); k.cs = cs;
    k.ar = fog->albedo[0]; k.ag = fog->albedo[1]; k.ab = fog->albedo[2]; k.ambient = fog->ambient;
    const uint32_t blocks = (uint32_t)(cells / 64);
    if (o32) hipLaunchKernelGGL(kfog_build<true>, dim3(blocks), dim3(64), 0, c->stream, k, set);
    else hipLaunchKernelGGL(kfog_build<false>, dim3(blocks), dim3(64), 0, c->stream, k, set);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "build_fog");
    f.path = o32 ? 32 : 64;
    if ((e = tables_leave(c)) != hipSuccess) return lhip(c, e, "build_fog: event record");
    f.m = m; f.level = fog->level;
    f.epoch = c->grid_epoch; f.serial = g.mips_serial;
    f.built = true;
    return VCT_OK;
}

extern "C" vct_status vct_fog_dims(const vct_ctx* c, uint32_t* m) {
    if (!c || !m) return VCT_EINVAL;
    if (!fog_current(c)) return VCT_ESTATE;
    *m = c->fog.m;
    return VCT_OK;
}

extern "C" vct_status vct_download_fog(vct_ctx* c, float* host_rgba) {
    if (!c) return VCT_EINVAL;
    if (!host_rgba) return lfail(c, VCT_EINVAL, "download_fog: NULL buffer");
    if (!fog_current(c)) return lfail(c, VCT_ESTATE, "download_fog without a current fog volume");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    const Fog& f = c->fog;
    const size_t cells = (size_t)f.m * f.m * f.m;
    std::vector<float4> tmp(cells);
    if ((e = hipMemcpyAsync(tmp.data(), f.vol, cells * sizeof(float4), hipMemcpyDeviceToHost, c->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return lhip(c, e, "download_fog");
    float4* out = (float4*)host_rgba;
    size_t v = 0;
    for (uint32_t z = 0; z < f.m; ++z)
        for (uint32_t y = 0; y < f.m; ++y)
            for (uint32_t x = 0; x < f.m; ++x, ++v) std::memcpy(&out[v], &tmp[texel_index(x, y, z, f.m)], sizeof(float4));
    return VCT_OK;
}

extern "C" vct_status vct_fog_rays_device(vct_ctx* c, const vct_camera* cam, const float* eye, const float* pos4,
                                          uint32_t w, uint32_t h, float* ray4) {
    if (!c) return VCT_EINVAL;
    if (!pos4 || !ray4 || !eye || w == 0 || h == 0) return lfail(c, VCT_EINVAL, "fog_rays: NULL buffer or empty frame");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "fog_rays: frame too large");
    if ((((uintptr_t)pos4 | (uintptr_t)ray4) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "fog_rays: float4 buffers must be 16-byte aligned");
    const Grid& g = c->grid;
    float o[3];
    if (!fog_origin(g, eye, o)) return lfail(c, VCT_EINVAL, "fog_rays: eye must be finite");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    FogRayK k;
    std::memset(&k, 0, sizeof k);
    k.w = (int)w; k.h = (int)h;
    if (cam) camera_fields(k, cam, w, h);
    k.has_cam = cam ? 1 : 0;
    k.pos = (const float4*)pos4; k.ray = (float4*)ray4;
    k.ox = o[0]; k.oy = o[1]; k.oz = o[2];
    k.g0x = g.g0[0]; k.g0y = g.g0[1]; k.g0z = g.g0[2]; k.inv_h = g.inv_h;
    hipLaunchKernelGGL(kfog_rays, dim3((w * h + 255) / 256), dim3(256), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "fog_rays");
    return VCT_OK;
}

extern "C" vct_status vct_fog_march_device(vct_ctx* c, const vct_fog* fog, const float* eye, const float* ray4,
                                           uint32_t w, uint32_t h, float* fog4, unsigned long long* steps) {
    if (!c) return VCT_EINVAL;
    if (!fog) return lfail(c, VCT_EINVAL, "fog_march: NULL fog");
    if (!ray4 || !fog4 || !eye || w == 0 || h == 0) return lfail(c, VCT_EINVAL, "fog_march: NULL buffer or empty frame");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "fog_march: frame too large");
    if ((((uintptr_t)ray4 | (uintptr_t)fog4) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "fog_march: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)steps & 7u) != 0) return lfail(c, VCT_EINVAL, "fog_march: steps must be 8-byte aligned");
    const Grid& g = c->grid;
    float sigma = 0.0f, o[3];
    if (const char* bad = check_fog(g, *fog, sigma)) return lfail(c, VCT_EINVAL, std::string("fog_march: ") + bad);
    if (!fog_origin(g, eye, o)) return lfail(c, VCT_EINVAL, "fog_march: eye must be finite");
    if (!fog_current(c)) return lfail(c, VCT_ESTATE, "fog_march without a current fog volume (vct_build_fog)");
    const Fog& f = c->fog;
    if (f.level != fog->level) return lfail(c, VCT_ESTATE, "fog_march: the volume was built at another level");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    FogMarchK k;
    std::memset(&k, 0, sizeof k);
    k.ray = (const float4*)ray4; k.out = (float4*)fog4; k.steps_total = steps;
    k.vol = f.vol;
    k.vol_bytes = (uint32_t)((size_t)f.m * f.m * f.m * sizeof(float4));
    k.w = (int)w; k.h = (int)h; k.tiles_x = (int)((w + 7) / 8);
    k.m = (int)f.m; k.lgm = __builtin_ctz(f.m);
    k.nf = (float)g.n; k.ox = o[0]; k.oy = o[1]; k.oz = o[2];
    const float cs = exp2_level(fog->level);
    k.sigma = sigma; k.ds = fog->step * cs; k.inv_cs = 1.0f / cs;
    const uint32_t blocks = (uint32_t)k.tiles_x * ((h + 7) / 8);
    hipLaunchKernelGGL(kfog_march, dim3(blocks), dim3(64), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "fog_march");
    return VCT_OK;
}

extern "C" vct_status vct_fog_apply_device(vct_ctx* c, const float* fog4, uint32_t w, uint32_t h, float* linear4_inout,
                                           uint32_t* out_rgba8) {
    if (!c) return VCT_EINVAL;
    if (!fog4 || w == 0 || h == 0) return lfail(c, VCT_EINVAL, "fog_apply: NULL buffer or empty frame");
    if (!linear4_inout && !out_rgba8) return lfail(c, VCT_EINVAL, "fog_apply: no output");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "fog_apply: frame too large");
    if ((((uintptr_t)fog4 | (uintptr_t)linear4_inout) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "fog_apply: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)out_rgba8 & 3u) != 0) return lfail(c, VCT_EINVAL, "fog_apply: rgba8 buffer must be 4-byte aligned");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    FogApplyK k;
    k.fog = (const float4*)fog4; k.lin = (float4*)linear4_inout; k.rgba8 = out_rgba8; k.npx = w * h;
    hipLaunchKernelGGL(kfog_apply, dim3((k.npx + 255) / 256), dim3(256), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "fog_apply");
    return VCT_OK;
}

// Test and tool hook (not part of the public headers).  force64 >= 0: nonzero sends the light
// cones of every grid's fog build through the 64-bit-address path that 1024^3 takes
// (process-wide).  -> the address path of the context's last build: 32, 64, or 0 before any.
// set_counters != 0 (with a context): the following builds add the steps of their light cones to
// *light_steps and those of the ambient K4 launch to *ambient_steps (device counters, 8-byte
// aligned; NULL: not counted -- a counted K4 launch runs K4's counting form).
extern "C" int vct_debug_fog(vct_ctx* c, int force64, int set_counters, unsigned long long* light_steps,
                             unsigned long long* ambient_steps) {
    if (force64 >= 0) g_fog_force64.store(force64 ? 1 : 0);
    if (c && set_counters) {
        c->fog.dbg_light_steps = light_steps;
        c->fog.dbg_ambient_steps = ambient_steps;
    }
    return c ? c->fog.path : -1;
}
