// vct_shadow.hip — cone-traced soft shadows (include/vct_shadow.h; the arithmetic is
// include/vct_spec.h "shadow cones"): V for every (light, pixel), and the composite that
// reads it.
//
//   ks_steps    one lane per new aperture: the (t, D, l0, fr) rows of A.6 for that tau, the
//               recurrence of build_step_table run on the device so that no call copies
//               from host memory.  A context keeps one table per distinct tau it has met
//               (scratch slot 10, kShadowRows rows each); a table is written once.  A call
//               queued on another stream than the previous one first waits (on the device)
//               for that call's end, so the shared tables are never read before they are
//               built nor rewritten under a running march (tables_enter / tables_leave).
//   ks_march    one wave per 8x8 pixel block, one lane per pixel, the lights in a
//               wave-uniform loop with their constants in the kernel arguments.  A light no
//               lane of the wave needs is skipped on a ballot.  A hard light (tan_half 0)
//               is the plain voxel walk (dda_lim).  A soft light marches all lanes in
//               lockstep: step i is the same (t, D, l0, fr) for every lane, read with
//               v_readlane from the 64 rows the wave holds (lane r keeps row i0 + r; the
//               next 64 rows are fetched every 64 steps, which at 256^3 only apertures
//               below ~0.09 need), so the level, its buffer resource and the blend branch
//               are scalar.
//               A lane that has ended (alpha stop, light reached, left the grid) only drops
//               out of a mask -- an AND of compares -- and its loads are sent out of range;
//               the loop ends when a ballot finds no lane left.  Only alpha is read: 4-byte
//               loads of the texels' .w, 8 per level at level 0 / isotropic, 24 above.
//   ks_composite kl_composite (vct_lights.hip) with V read from the vis plane.
//
// n <= 512: every level is bound as a buffer resource (base at the first texel's .w), so
// the spec's zero border is the hardware range check.  n = 1024 (and vct_debug_shadow's
// force64): 64-bit addresses and an explicit select.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstring>
#include "vct_internal.h"
#include "vct_light_terms.h"

namespace vct {
namespace {

// rows per step table, the +inf sentinel included: VCT_SPEC_TAU_MIN on 1024^3 needs 265
constexpr int kShadowRows = 320;
constexpr int kSlotTabs = 10;            // vct_ctx::scratch
constexpr uint32_t kHard = 0xffu;        // ShadowK::slot of a light with tan_half 0
constexpr uint32_t kOutT = 0x0fffffffu;  // texel index of a corner outside its level: << 4 is past any level

struct alignas(16) AlphaRange {
    const float* base;           // &level[0].w
    uint32_t bytes;              // from there to the level's end (every face); 0: not bound (64-bit path)
    uint32_t pad;
};

struct ShadowK {
    const float4* pos;
    const float4* nrm;
    const unsigned long long* bits;
    const StepRow* tabs;         // [slot][kShadowRows]
    float* vis;                  // [n_lights][h][w]
    unsigned long long* steps_total;
    AlphaRange lvl[kMaxLevels + 1];
    int n, L, lgn, aniso;
    int w, h, tiles_x;
    uint32_t n_lights;
    float g0x, g0y, g0z, inv_h, h2, tmax;
    uint8_t slot[VCT_MAX_LIGHTS];    // the light's step table, kHard: the voxel walk
};

struct StepsK {
    float tau[VCT_MAX_LIGHTS];
    uint32_t first, count;       // tables [first, first + count)
    float tmax, Lf;
    StepRow* tabs;
};

__global__ void __launch_bounds__(64) ks_steps(const StepsK k) {
    if (threadIdx.x >= k.count) return;
    StepRow* const rows = k.tabs + (size_t)(k.first + threadIdx.x) * kShadowRows;
    const float tau2 = 2.0f * k.tau[threadIdx.x];
    float t = 1.0f;
    for (int i = 0; i < kShadowRows; ++i) {
        if (!(t <= k.tmax)) {
            rows[i] = StepRow{__builtin_inff(), 1.0f, 0.0f, 0};
            continue;                                  // the rest of the table is the sentinel
        }
        const float D = fmaxf(1.0f, tau2 * t);
        float m = spec_log2(D);
        if (m > k.Lf) m = k.Lf;
        const int l0 = (int)m;
        rows[i] = StepRow{t, D, m - (float)l0, l0};
        t = t + VCT_STEP_SCALE * D;
    }
}

// coordinates c and c + 1 of one axis of a level of nl = 2^lg texels, as OR-able fields of
// the brick layout's texel index (vct_device.h texel_index): (c >> 1) << sh | (c & 1) << bit
struct Axis {
    uint32_t t0, t1;
    bool in0, in1;
};
__device__ __forceinline__ Axis axis_fields(int c, uint32_t nl, uint32_t sh, uint32_t bit) {
    const uint32_t u = (uint32_t)c, v = u + 1u;
    return Axis{((u >> 1) << sh) | ((u & 1u) << bit), ((v >> 1) << sh) | ((v & 1u) << bit), u < nl, v < nl};
}

// the alpha of D_l(p, d) (A.5) for a wave-uniform level l; `act`: the lane still marches (an
// ended lane reads nothing).  fx, fy, fz: the faces d selects; wdx, wdy, wdz: d_c^2.
template <bool O32>
__device__ __forceinline__ float sample_alpha(const ShadowK& k, int l, bool act, float px, float py, float pz, int fx,
                                              int fy, int fz, float wdx, float wdy, float wdz) {
    const float scale = __uint_as_float((uint32_t)(127 - l) << 23);   // 2^-l, exact
    const float cx = px * scale - 0.5f, cy = py * scale - 0.5f, cz = pz * scale - 0.5f;
    const float flx = floorf(cx), fly = floorf(cy), flz = floorf(cz);
    const float ax = cx - flx, ay = cy - fly, az = cz - flz;
    const float wx[2] = {1.0f - ax, ax}, wy[2] = {1.0f - ay, ay}, wz[2] = {1.0f - az, az};
    const uint32_t lg = (uint32_t)(k.lgn - l), lnb = lg > 0u ? lg - 1u : 0u, nl = 1u << lg;
    const Axis X = axis_fields((int)flx, nl, 3u, 0u), Y = axis_fields((int)fly, nl, lnb + 3u, 1u),
               Z = axis_fields((int)flz, nl, 2u * lnb + 3u, 2u);
    const bool faces = l != 0 && k.aniso;
    const uint32_t shf = 3u * lg;                                      // face f starts at texel f << shf
    const AlphaRange r = k.lvl[l];
    float acc = 0.0f;
    if constexpr (O32) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)r.base, (short)0, (int)r.bytes, 0x00020000);
        const uint32_t xs[2] = {act && X.in0 ? X.t0 : kOutT, act && X.in1 ? X.t1 : kOutT};
        const uint32_t ys[2] = {Y.in0 ? Y.t0 : kOutT, Y.in1 ? Y.t1 : kOutT};
        const uint32_t zs[2] = {Z.in0 ? Z.t0 : kOutT, Z.in1 ? Z.t1 : kOutT};
        const auto ld = [&](uint32_t texel) {
            return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, texel << 4, 0, 0));
        };
        if (!faces) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = ld(xs[c & 1] | ys[(c >> 1) & 1] | zs[c >> 2]);
#pragma unroll
            for (int c = 0; c < 8; ++c) acc = fmaf((wx[c & 1] * wy[(c >> 1) & 1]) * wz[c >> 2], v[c], acc);
            return acc;
        }
        const uint32_t FX = (uint32_t)fx << shf, FY = (uint32_t)fy << shf, FZ = (uint32_t)fz << shf;
        float vx[8], vy[8], vz[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t t = xs[c & 1] | ys[(c >> 1) & 1] | zs[c >> 2];
            vx[c] = ld(t | FX);
            vy[c] = ld(t | FY);
            vz[c] = ld(t | FZ);
        }
#pragma unroll
        for (int c = 0; c < 8; ++c)
            acc = fmaf((wx[c & 1] * wy[(c >> 1) & 1]) * wz[c >> 2], fmaf(wdz, vz[c], fmaf(wdy, vy[c], wdx * vx[c])), acc);
        return acc;
    } else {
        const float* const base = r.base;
        const auto ld = [&](uint32_t texel, bool in) {
            const float v = base[(size_t)(in ? texel : 0u) << 2];
            return in ? v : 0.0f;
        };
        const uint32_t xs[2] = {X.t0, X.t1}, ys[2] = {Y.t0, Y.t1}, zs[2] = {Z.t0, Z.t1};
        const bool ix[2] = {act && X.in0, act && X.in1}, iy[2] = {Y.in0, Y.in1}, iz[2] = {Z.in0, Z.in1};
        const uint32_t FX = faces ? (uint32_t)fx << shf : 0u, FY = (uint32_t)fy << shf, FZ = (uint32_t)fz << shf;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t t = xs[c & 1] | ys[(c >> 1) & 1] | zs[c >> 2];
            const bool in = ix[c & 1] && iy[(c >> 1) & 1] && iz[c >> 2];
            float v = ld(t | FX, in);
            if (faces) v = fmaf(wdz, ld(t | FZ, in), fmaf(wdy, ld(t | FY, in), wdx * v));
            acc = fmaf((wx[c & 1] * wy[(c >> 1) & 1]) * wz[c >> 2], v, acc);
        }
        return acc;
    }
}

__device__ __forceinline__ float lane_row(float v, int r) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r));
}

// one shadow cone per lane, the wave in lockstep ("shadow cones" 1-5); returns a.
// `need`: the lane marches at all.  The direction is per lane; for a directional light the
// caller passes the light's own (scalar) l, and the faces and d^2 below stay scalar.
template <bool O32>
__device__ __forceinline__ float cone(const ShadowK& k, const StepRow* __restrict__ tab, bool need, float ox, float oy,
                                      float oz, float dx, float dy, float dz, float t_lim, uint32_t& steps) {
    const float nf = (float)k.n;
    const int fx = dx >= 0.0f ? VCT_FACE_PX : VCT_FACE_NX;
    const int fy = dy >= 0.0f ? VCT_FACE_PY : VCT_FACE_NY;
    const int fz = dz >= 0.0f ? VCT_FACE_PZ : VCT_FACE_NZ;
    const float wdx = dx * dx, wdy = dy * dy, wdz = dz * dz;
    float a = 0.0f;
    bool act = need;
    StepRow row{};
    for (int i = 0; i < kShadowRows; ++i) {
        const int r = i & 63;
        if (r == 0) row = tab[i + (int)threadIdx.x];          // rows i .. i + 63, lane r keeps row i + r
        const float t = lane_row(row.t, r);
        if (!(t <= k.tmax)) break;                             // the sentinel: every lane ends
        const float px = ox + dx * t, py = oy + dy * t, pz = oz + dz * t;
        act = act & (a < VCT_ALPHA_STOP) & !(t >= t_lim) &
              ((px >= 0.0f) & (px <= nf) & (py >= 0.0f) & (py <= nf) & (pz >= 0.0f) & (pz <= nf));
        if (__builtin_amdgcn_ballot_w64(act) == 0ull) break;
        const int l0 = __builtin_amdgcn_readlane(row.l0, r);
        const float fr = lane_row(row.fr, r);
        float s = sample_alpha<O32>(k, l0, act, px, py, pz, fx, fy, fz, wdx, wdy, wdz);
        if (fr > 0.0f && l0 < k.L) {
            const float s1 = sample_alpha<O32>(k, l0 + 1, act, px, py, pz, fx, fy, fz, wdx, wdy, wdz);
            s = fmaf(fr, s1, (1.0f - fr) * s);
        }
        const float oma = 1.0f - a;
        a = act ? fmaf(oma, s, a) : a;
        steps += act ? 1u : 0u;
    }
    return a;
}

template <bool O32>
__global__ void __launch_bounds__(64) ks_march(const ShadowK k, const LightSet set) {
    const int lane = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / k.tiles_x, tx = (int)blockIdx.x - ty * k.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const bool inframe = x < k.w && y < k.h;
    const size_t npx = (size_t)k.w * (size_t)k.h;
    const size_t i = inframe ? (size_t)y * (size_t)k.w + (size_t)x : 0u;
    const float4 P = k.pos[i], N = k.nrm[i];
    const bool valid = inframe && P.w != 0.0f;
    const float qx = (P.x - k.g0x) * k.inv_h + N.x, qy = (P.y - k.g0y) * k.inv_h + N.y,
                qz = (P.z - k.g0z) * k.inv_h + N.z;
    uint32_t steps = 0;
    for (uint32_t j = 0; j < k.n_lights; ++j) {
        const DLight& L = set.l[j];
        float lx = 0.0f, ly = 0.0f, lz = 0.0f, f, ndl, t_lim = 0.0f;
        const bool need = valid && light_terms(L, k.h2, qx, qy, qz, N.x, N.y, N.z, lx, ly, lz, f, ndl, t_lim);
        float V = 0.0f;
        if (__builtin_amdgcn_ballot_w64(need) != 0ull) {
            const uint32_t slot = k.slot[j];
            if (slot == kHard) {
                if (need) V = dda_lim(k.bits, k.n, qx, qy, qz, lx, ly, lz, t_lim);
            } else {
                const StepRow* tab = k.tabs + (size_t)slot * kShadowRows;
                float a;
                if (L.type == VCT_LIGHT_DIRECTIONAL)   // l is the light's: faces and d^2 are scalar
                    a = cone<O32>(k, tab, need, qx, qy, qz, L.ax, L.ay, L.az, __builtin_inff(), steps);
                else
                    a = cone<O32>(k, tab, need, qx, qy, qz, lx, ly, lz, t_lim, steps);
                V = fmaxf(1.0f - a / VCT_ALPHA_STOP, 0.0f);
            }
        }
        if (inframe) k.vis[(size_t)j * npx + i] = need ? V : 0.0f;
    }
    if (k.steps_total) {
        const uint32_t ws = wave_sum_u32(steps);
        if (lane == 0 && ws) atomicAdd(k.steps_total, (unsigned long long)ws);
    }
}

// ---- composite + present with V from the vis plane (kl_composite, vct_lights.hip) -------
struct CompVK {
    const float4 *pos, *nrm, *alb, *diff, *spec;
    const float* vis;
    int w, h;
    float g0x, g0y, g0z, inv_h, h2;
    uint32_t n_lights;
    float4* lin;
    uint32_t* rgba8;
};

__global__ void __launch_bounds__(256) ks_composite(const CompVK k, const LightSet set) {
    const uint32_t npx = (uint32_t)k.w * (uint32_t)k.h;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npx) return;
    const float4 P = k.pos[i];
    if (P.w == 0.0f) {   // background: the reference's clear colour
        if (k.lin) k.lin[i] = make_float4(VCT_CLEAR_R, VCT_CLEAR_G, VCT_CLEAR_B, 0.0f);
        if (k.rgba8)
            k.rgba8[i] = (uint32_t)lroundf(VCT_CLEAR_R * 255.0f) | ((uint32_t)lroundf(VCT_CLEAR_G * 255.0f) << 8) |
                         ((uint32_t)lroundf(VCT_CLEAR_B * 255.0f) << 16) | (255u << 24);
        return;
    }
    const float4 N = k.nrm[i], A = k.alb[i], D = k.diff[i], S = k.spec[i];
    const float qx = (P.x - k.g0x) * k.inv_h + N.x, qy = (P.y - k.g0y) * k.inv_h + N.y,
                qz = (P.z - k.g0z) * k.inv_h + N.z;
    float dr = 0.0f, dg = 0.0f, db = 0.0f;
    for (uint32_t j = 0; j < k.n_lights; ++j) {
        const DLight& L = set.l[j];
        float lx, ly, lz, f, ndl, t_lim;
        if (!light_terms(L, k.h2, qx, qy, qz, N.x, N.y, N.z, lx, ly, lz, f, ndl, t_lim)) continue;
        const float vis = k.vis[(size_t)j * npx + i];
        dr = dr + (((A.x * L.cr) * ndl) * f) * vis;
        dg = dg + (((A.y * L.cg) * ndl) * f) * vis;
        db = db + (((A.z * L.cb) * ndl) * f) * vis;
    }
    const float fr = (dr + A.x * D.x) + S.x, fg = (dg + A.y * D.y) + S.y, fb = (db + A.z * D.z) + S.z;
    if (k.lin) k.lin[i] = make_float4(fr, fg, fb, 1.0f);
    if (k.rgba8) k.rgba8[i] = to8(fr) | (to8(fg) << 8) | (to8(fb) << 16) | (255u << 24);
}

// ---- host side --------------------------------------------------------------------------
std::atomic<int> g_force64{0};   // vct_debug_shadow: every grid takes the 64-bit path

// rows of tau's table, the sentinel included (the t recurrence of ks_steps; log2 is not needed)
int table_rows(float tau, float tmax) {
    const float tau2 = 2.0f * tau;
    float t = 1.0f;
    int i = 0;
    for (; i < kShadowRows && t <= tmax; ++i) t = t + VCT_STEP_SCALE * fmaxf(1.0f, tau2 * t);
    return t <= tmax ? kShadowRows + 1 : i + 1;
}

// slot[j] = the step table of light j's aperture (kHard for tan_half 0), building what the
// context does not hold yet.  A table is never rewritten while the context keeps it; when
// the 64 slots are used up, the set starts again from this call's apertures.  The caller has
// ordered the ctx stream after the previous call's march (tables_enter), so both the build
// and the restart are safe whatever streams the calls come on.
vct_status step_tables(vct_ctx* c, const float* tan_half, uint32_t n_lights, uint8_t* slot, const StepRow** tabs) {
    const Grid& g = c->grid;
    const float tmax = (float)g.n * VCT_SQRT3;
    float tau[VCT_MAX_LIGHTS];
    for (uint32_t j = 0; j < n_lights; ++j)
        tau[j] = tan_half[j] == 0.0f ? 0.0f : fminf(fmaxf(tan_half[j], VCT_SPEC_TAU_MIN), VCT_SPEC_TAU_MAX);
    void* p = nullptr;
    hipError_t e = scratch_get(c, kSlotTabs, sizeof(StepRow) * kShadowRows * VCT_MAX_LIGHTS, &p);
    if (e != hipSuccess) return lhip(c, e, "shadow_cones: step tables");
    *tabs = (const StepRow*)p;
    for (int pass = 0; pass < 2; ++pass) {
        uint32_t have = c->shadow_taus, first = have;
        bool fits = true;
        for (uint32_t j = 0; j < n_lights && fits; ++j) {
            slot[j] = (uint8_t)kHard;
            if (tau[j] == 0.0f) continue;
            uint32_t s = 0;
            while (s < have && std::memcmp(&c->shadow_tau[s], &tau[j], 4) != 0) ++s;
            if (s == have) {
                if (have == VCT_MAX_LIGHTS) { fits = false; break; }
                if (table_rows(tau[j], tmax) > kShadowRows)
                    return lfail(c, VCT_EINVAL, "shadow_cones: the aperture needs more step rows than a table holds");
                c->shadow_tau[have++] = tau[j];
            }
            slot[j] = (uint8_t)s;
        }
        if (!fits) {             // start the set again (at most 64 apertures per call: the second pass fits)
            c->shadow_taus = 0;
            continue;
        }
        if (have > first) {
            StepsK sk;
            std::memset(&sk, 0, sizeof sk);
            std::memcpy(sk.tau, c->shadow_tau + first, (have - first) * sizeof(float));
            sk.first = first; sk.count = have - first;
            sk.tmax = tmax; sk.Lf = (float)g.L;
            sk.tabs = (StepRow*)p;
            hipLaunchKernelGGL(ks_steps, dim3(1), dim3(64), 0, c->stream, sk);
            if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "shadow_cones: step tables");
            c->shadow_taus = have;
        }
        return VCT_OK;
    }
    return lfail(c, VCT_EINVAL, "shadow_cones: step tables");
}

// Order this call after the previous vct_shadow_cones_device of the context when that one was
// queued on another stream (vct_ctx::shadow_done), and mark this call's end.
hipError_t tables_enter(vct_ctx* c) {
    if (c->shadow_done && c->shadow_stream != c->stream) return hipStreamWaitEvent(c->stream, c->shadow_done, 0);
    return hipSuccess;
}

hipError_t tables_leave(vct_ctx* c) {
    if (!c->shadow_done) {
        hipError_t e = hipEventCreateWithFlags(&c->shadow_done, hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    c->shadow_stream = c->stream;
    return hipEventRecord(c->shadow_done, c->stream);
}

}  // namespace
}  // namespace vct

using namespace vct;

extern "C" vct_status vct_shadow_cones_device(vct_ctx* c, const float* pos4, const float* nrm4, uint32_t w, uint32_t h,
                                              const vct_light* lights, uint32_t n_lights, const float* tan_half,
                                              float* vis, unsigned long long* cone_steps) {
    if (!c) return VCT_EINVAL;
    if (!pos4 || !nrm4 || !vis || w == 0 || h == 0) return lfail(c, VCT_EINVAL, "shadow_cones: NULL buffer or empty frame");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "shadow_cones: frame too large");
    if ((((uintptr_t)pos4 | (uintptr_t)nrm4) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "shadow_cones: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)vis & 3u) != 0) return lfail(c, VCT_EINVAL, "shadow_cones: vis must be 4-byte aligned");
    if (((uintptr_t)cone_steps & 7u) != 0) return lfail(c, VCT_EINVAL, "shadow_cones: cone_steps must be 8-byte aligned");
    if (n_lights > VCT_MAX_LIGHTS) return lfail(c, VCT_EINVAL, "shadow_cones: more than VCT_MAX_LIGHTS lights");
    if (n_lights && !tan_half) return lfail(c, VCT_EINVAL, "shadow_cones: NULL tan_half");
    for (uint32_t j = 0; j < n_lights; ++j)
        if (!std::isfinite(tan_half[j]) || tan_half[j] < 0.0f)
            return lfail(c, VCT_EINVAL, "shadow_cones: tan_half[" + std::to_string(j) + "] must be finite and >= 0");
    const Grid& g = c->grid;
    if (!g.voxelized || !g.mipped) return lfail(c, VCT_ESTATE, "shadow_cones before voxelize / build_mips");
    LightSet set;
    std::memset(&set, 0, sizeof set);
    vct_status st = prepare_list(c, "shadow_cones", lights, n_lights, set.l);
    if (st != VCT_OK) return st;
    if (n_lights == 0) return VCT_OK;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    ShadowK k;
    std::memset(&k, 0, sizeof k);
    if ((e = tables_enter(c)) != hipSuccess) return lhip(c, e, "shadow_cones: stream wait");
    if ((st = step_tables(c, tan_half, n_lights, k.slot, &k.tabs)) != VCT_OK) return st;
    const bool o32 = g.n <= 512 && !g_force64.load();
    for (int i = 0; i <= (int)g.L; ++i) {
        const uint64_t ni = (uint64_t)(g.n >> i);
        const uint64_t by = ni * ni * ni * 16u * (i > 0 && g.aniso ? 6u : 1u);
        k.lvl[i] = AlphaRange{(const float*)(g.pyr + g.lvl_off[i]) + 3, o32 ? (uint32_t)(by - 12u) : 0u, 0u};
    }
    k.pos = (const float4*)pos4; k.nrm = (const float4*)nrm4;
    k.bits = g.occ_bits;
    k.vis = vis; k.steps_total = cone_steps;
    k.n = (int)g.n; k.L = (int)g.L; k.lgn = __builtin_ctz(g.n); k.aniso = g.aniso;
    k.w = (int)w; k.h = (int)h; k.tiles_x = (int)((w + 7) / 8);
    k.n_lights = n_lights;
    k.g0x = g.g0[0]; k.g0y = g.g0[1]; k.g0z = g.g0[2]; k.inv_h = g.inv_h; k.h2 = grid_h2(g);
    k.tmax = (float)g.n * VCT_SQRT3;
    const uint32_t blocks = (uint32_t)k.tiles_x * ((h + 7) / 8);
    if (o32) hipLaunchKernelGGL(ks_march<true>, dim3(blocks), dim3(64), 0, c->stream, k, set);
    else hipLaunchKernelGGL(ks_march<false>, dim3(blocks), dim3(64), 0, c->stream, k, set);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "shadow_cones");
    c->shadow_path = o32 ? 32 : 64;
    if ((e = tables_leave(c)) != hipSuccess) return lhip(c, e, "shadow_cones: event record");
    return VCT_OK;
}

extern "C" vct_status vct_composite_shadowed_device(vct_ctx* c, const float* pos4, const float* nrm4, const float* alb4,
                                                    const float* diffuse4, const float* spec4, uint32_t w, uint32_t h,
                                                    const vct_light* lights, uint32_t n_lights, const float* vis,
                                                    float* out_linear4, uint32_t* out_rgba8) {
    if (!c || !pos4 || !nrm4 || !alb4 || !diffuse4 || !spec4 || w == 0 || h == 0) return VCT_EINVAL;
    if (!out_linear4 && !out_rgba8) return lfail(c, VCT_EINVAL, "composite: no output");
    if ((uint64_t)w * h > 0x7fffffffull) return lfail(c, VCT_EINVAL, "composite: frame too large");
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "composite before voxelize");
    for (const void* p : {(const void*)pos4, (const void*)nrm4, (const void*)alb4, (const void*)diffuse4,
                          (const void*)spec4, (const void*)out_linear4})
        if (((uintptr_t)p & 15u) != 0) return lfail(c, VCT_EINVAL, "composite: float4 buffers must be 16-byte aligned");
    if (((uintptr_t)out_rgba8 & 3u) != 0) return lfail(c, VCT_EINVAL, "composite: rgba8 buffer must be 4-byte aligned");
    if (n_lights && n_lights <= VCT_MAX_LIGHTS && (!vis || ((uintptr_t)vis & 3u) != 0))
        return lfail(c, VCT_EINVAL, "composite_shadowed: vis must be a 4-byte aligned device buffer");
    LightSet set;
    std::memset(&set, 0, sizeof set);
    vct_status st = prepare_list(c, "composite_shadowed", lights, n_lights, set.l);
    if (st != VCT_OK) return st;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    const Grid& g = c->grid;
    CompVK k;
    k.pos = (const float4*)pos4; k.nrm = (const float4*)nrm4; k.alb = (const float4*)alb4;
    k.diff = (const float4*)diffuse4; k.spec = (const float4*)spec4;
    k.vis = vis;
    k.w = (int)w; k.h = (int)h;
    k.g0x = g.g0[0]; k.g0y = g.g0[1]; k.g0z = g.g0[2]; k.inv_h = g.inv_h; k.h2 = grid_h2(g);
    k.n_lights = n_lights;
    k.lin = (float4*)out_linear4; k.rgba8 = out_rgba8;
    hipLaunchKernelGGL(ks_composite, dim3((w * h + 255) / 256), dim3(256), 0, c->stream, k, set);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "composite_shadowed");
    return VCT_OK;
}

// Test hook (not part of the public headers): force64 != 0 sends every grid through the
// 64-bit-address path that 1024^3 takes.  Process-wide.
extern "C" void vct_debug_shadow(int force64) { g_force64.store(force64 ? 1 : 0); }

// The address path the context's last vct_shadow_cones_device march was launched with: 32
// (buffer resources), 64 (64-bit addresses), 0 before the first one.
extern "C" int vct_debug_shadow_path(const vct_ctx* c) { return c ? c->shadow_path : -1; }
