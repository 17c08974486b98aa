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
// The composite that reads V is kl_composite<true, *> (vct_lights.hip);
// vct_composite_shadowed_device here keeps its own rule (vis is required).
//
// n <= 512: every level is bound as a buffer resource (base at the first texel's .w), so
// the spec's zero border is the hardware range check.  n = 1024 (and vct_debug_shadow's
// force64): 64-bit addresses and an explicit select.
//
// The march itself (the step rows a wave holds, the alpha sample with both address paths,
// the lockstep cone) is csrc/vct_alpha_march.h, shared with vct_sky.hip; this unit keeps the
// context's table set (ks_steps, step_tables, tables_enter / tables_leave), which the sky
// calls go through as well.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstring>
#include "vct_internal.h"
#include "vct_light_terms.h"
#include "vct_alpha_march.h"

namespace vct {
namespace {

constexpr int kSlotTabs = 10;            // vct_ctx::scratch
constexpr uint32_t kHard = kHardSlot;    // ShadowK::slot of a light with tan_half 0

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
                // shadow-walk receiver rule (vct_spec.h): outside the float test V = 1, as the
                // soft path's cone gives for the same pixel (0 steps)
                if (need)
                    V = walk_starts(k.n, qx, qy, qz) ? dda_lim(k.bits, k.n, qx, qy, qz, lx, ly, lz, t_lim) : 1.0f;
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

}  // namespace

// the context's step tables (vct_alpha_march.h has the contract)
vct_status step_tables(vct_ctx* c, const char* what, const float* tan_half, uint32_t n_lights, uint8_t* slot,
                       const StepRow** tabs) {
    const std::string where = std::string(what) + ": step tables";
    const Grid& g = c->grid;
    const float tmax = (float)g.n * VCT_SQRT3;
    float tau[VCT_MAX_LIGHTS];
    for (uint32_t j = 0; j < n_lights; ++j)
        tau[j] = tan_half[j] == 0.0f ? 0.0f : fminf(fmaxf(tan_half[j], VCT_SPEC_TAU_MIN), VCT_SPEC_TAU_MAX);
    void* p = nullptr;
    hipError_t e = scratch_get(c, kSlotTabs, sizeof(StepRow) * kShadowRows * VCT_MAX_LIGHTS, &p);
    if (e != hipSuccess) return lhip(c, e, where.c_str());
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
                    return lfail(c, VCT_EINVAL, std::string(what) + ": the aperture needs more step rows than a table holds");
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
            if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, where.c_str());
            c->shadow_taus = have;
        }
        return VCT_OK;
    }
    return lfail(c, VCT_EINVAL, where);
}

// Order this call after the context's previous march over the tables (a shadow or a sky call)
// when that one was queued on another stream (vct_ctx::shadow_done), and mark this call's end.
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
    if ((st = step_tables(c, "shadow_cones", tan_half, n_lights, k.slot, &k.tabs)) != VCT_OK) return st;
    const bool o32 = g.n <= 512 && !g_force64.load();
    alpha_ranges(g, o32, k.lvl);
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
    // vis is needed when a light reads it (a list that is too long is the list check's to report)
    CompositeForm form;
    form.vis = vis;
    form.read_vis = true;
    if (n_lights && n_lights <= VCT_MAX_LIGHTS && (!vis || ((uintptr_t)vis & 3u) != 0))
        form.own_error = "vis must be a 4-byte aligned device buffer";
    return composite_light_list(c, "composite_shadowed", pos4, nrm4, alb4, diffuse4, spec4, w, h, lights, n_lights, form,
                                out_linear4, out_rgba8);
}

// Test hook (not part of the public headers): force64 != 0 sends every grid through the
// 64-bit-address path that 1024^3 takes.  Process-wide.
extern "C" void vct_debug_shadow(int force64) { g_force64.store(force64 ? 1 : 0); }

// The address path the context's last vct_shadow_cones_device march was launched with: 32
// (buffer resources), 64 (64-bit addresses), 0 before the first one.
extern "C" int vct_debug_shadow_path(const vct_ctx* c) { return c ? c->shadow_path : -1; }
