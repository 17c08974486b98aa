// vct_alpha_march.h — the alpha-only cone march that vct_shadow.hip (one cone per light and
// pixel) and vct_sky_march.h (the diffuse cone set per receiver, the specular cone per pixel)
// share: the step rows a wave holds, the alpha sample of one level with its two address
// paths, the lockstep march of vct_spec.h "shadow cones" steps 1-5 (cone<>), the same march
// with an aperture per lane (cone_lane<>), and the context's set of step tables.
//
// The device code is templated on the kernel's argument record K, which must have
//     AlphaRange lvl[kMaxLevels + 1];  int n, L, lgn, aniso;  float tmax;
// so each kernel keeps its own record layout.  Device code is internal to the including
// translation unit; the table set (one per context, scratch slot 10) lives in vct_shadow.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "vct_internal.h"

namespace vct {

// rows per step table, the +inf sentinel included: VCT_SPEC_TAU_MIN on 1024^3 needs 265
constexpr int kShadowRows = 320;

// ---- the context's step tables (defined in vct_shadow.hip) -------------------------------
// slot[j] = the step table of aperture tan_half[j] (kHardSlot for tan_half 0), building what
// the context does not hold yet.  A table is never rewritten while the context keeps it; when
// the 64 slots are used up, the set starts again from this call's apertures.  The caller has
// ordered the ctx stream after the previous march (tables_enter), so both the build and the
// restart are safe whatever streams the calls come on.  `what` names the caller in errors.
constexpr uint32_t kHardSlot = 0xffu;
vct_status step_tables(vct_ctx* c, const char* what, const float* tan_half, uint32_t n, uint8_t* slot,
                       const StepRow** tabs);
// Order this call after the context's previous march over the tables when that one was queued
// on another stream (vct_ctx::shadow_done), and mark this call's end.
hipError_t tables_enter(vct_ctx* c);
hipError_t tables_leave(vct_ctx* c);

namespace {

constexpr uint32_t kOutT = 0x0fffffffu;  // texel index of a corner outside its level: << 4 is past any level

struct alignas(16) AlphaRange {
    const float* base;           // &level[0].w
    uint32_t bytes;              // from there to the level's end (every face); 0: not bound (64-bit path)
    uint32_t pad;
};

// lvl[i] of a kernel record for the context's pyramid; o32: bound as buffer resources
inline void alpha_ranges(const Grid& g, bool o32, AlphaRange* lvl) {
    for (int i = 0; i <= (int)g.L; ++i) {
        const uint64_t ni = (uint64_t)(g.n >> i);
        const uint64_t by = ni * ni * ni * 16u * (i > 0 && g.aniso ? 6u : 1u);
        lvl[i] = AlphaRange{(const float*)(g.pyr + g.lvl_off[i]) + 3, o32 ? (uint32_t)(by - 12u) : 0u, 0u};
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
template <bool O32, class K>
__device__ __forceinline__ float sample_alpha(const K& k, int l, bool act, float px, float py, float pz, int fx,
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

// one alpha cone per lane, the wave in lockstep ("shadow cones" 1-5); returns a.
// `need`: the lane marches at all.  The direction is per lane; a caller whose direction is
// the same for every lane passes it as scalars, and the faces and d^2 below stay scalar.
// Step i is the same (t, D, l0, fr) for every lane, read with v_readlane from the 64 rows
// the wave holds (lane r keeps row i0 + r; the next 64 rows are fetched every 64 steps).
template <bool O32, class K>
__device__ __forceinline__ float cone(const K& k, const StepRow* __restrict__ tab, bool need, float ox, float oy,
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

// one alpha cone per lane, each lane with an aperture tau of its own ("shadow cones" 1-5 with
// t_lim = +inf); returns a.  No step table applies: every lane derives its steps in registers
// (t, D = max(1, 2 tau t), m = log2 D, l0, fr: K4's per-lane march).  sample_alpha wants a
// wave-uniform level, so a step loops over the levels present among the lanes that still
// march: the first pending lane's l0 is read onto the scalar unit, the lanes of that level
// sample and leave the pending mask.  A wave whose lanes share one tau has one t sequence and
// runs the loop once per step (the lockstep march, with no special case); a wave of mixed tau
// pays one pass per distinct level.  The second level of a step (fr > 0, l0 < L) is handled
// the same way.  Addresses: a lane outside the pass is an ended lane to sample_alpha, so its
// loads go past the buffer range (O32) or read texel 0 and select zero (64-bit); a lane inside
// it has a finite p in [0, n]^3 and 0 <= l <= L, the range sample_alpha's corners are checked
// against.  tau must be clamped to VCT_SPEC_TAU_MIN..MAX by the caller.
template <bool O32, class K>
__device__ __forceinline__ float cone_lane(const K& k, bool need, float ox, float oy, float oz, float dx, float dy,
                                           float dz, float tau, uint32_t& steps) {
    const float tau2 = 2.0f * tau;
    const float nf = (float)k.n, Lf = (float)k.L;
    const int fx = dx >= 0.0f ? VCT_FACE_PX : VCT_FACE_NX;
    const int fy = dy >= 0.0f ? VCT_FACE_PY : VCT_FACE_NY;
    const int fz = dz >= 0.0f ? VCT_FACE_PZ : VCT_FACE_NZ;
    const float wdx = dx * dx, wdy = dy * dy, wdz = dz * dz;
    float a = 0.0f, t = 1.0f;
    bool act = need;
    for (;;) {
        // step 1; t grows by at least 0.5 a step, so the loop ends
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
    return a;
}

}  // namespace
}  // namespace vct
