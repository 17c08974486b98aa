// vct_query.hip — cone queries and the ambient-cube probe grid (include/vct_query.h; the
// arithmetic is include/vct_spec.h "cone queries" and "probe grid").
//
//   kquery        one cone per lane, in list order: an arbitrary (origin, direction, aperture,
//                 limit) record marched through the RGBA pyramid by K4's rule.  Every lane has
//                 its own aperture, so it derives its own (t, D, l0, fr) in registers with the
//                 spec's log2, as cone_lane (vct_alpha_march.h) does; no step table applies.
//                 A step loops over the levels present among the lanes that still march: the
//                 first pending lane's level is read onto the scalar unit (so the level's base
//                 and shifts stay scalar), the lanes of that level sample under their own exec
//                 mask and leave the pending set.  The second level of a step (fr > 0, l0 < L)
//                 is handled the same way.  A wave of one aperture runs each loop once per step.
//   kprobe_build  the same march (the one device function, so the build equals the query bit
//                 for bit) over cones generated in registers: lane i is face i % 6 of probe
//                 i / 6; the face-0 lane also writes the probe's state from K1's occupancy bits.
//   kprobe_sample one point per lane: eight probes, three faces each.
//
// The level sample is the RGBA counterpart of vct_alpha_march.h's sample_alpha: eight corner
// texels as float4 loads at the brick layout's texel index (vct_device.h), three faces per
// corner on an anisotropic level above 0.  One address path: 64-bit addresses from the level's
// base (a 1024^3 anisotropic level is past a 32-bit buffer range).  A corner outside its level
// is not read.  No lane reads another lane's cone, and the only atomics are the wave-summed
// integer counters.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "vct_internal.h"
#include "vct_light_terms.h"

namespace vct {
namespace {

struct QueryGrid {
    const float4* lvl[kMaxLevels + 1];   // texel 0 of each level (face 0)
    int n, L, lgn, aniso;
    float g0x, g0y, g0z, inv_h, tmax;
};

struct QueryK {
    QueryGrid g;
    const float4* cones;                 // [count][3]
    float4* out;                         // [count]
    uint32_t* steps;                     // [count] or null
    unsigned long long* steps_total;     // or null
    uint32_t count;
};

struct ProbeBuildK {
    QueryGrid g;
    const unsigned long long* occ_bits;
    float4* probes;                      // [probes][6]
    uint32_t* state;                     // [probes]
    unsigned long long* steps_total;
    uint32_t dx, dy, dz, lanes;          // lanes = 6 * probes
    float ox, oy, oz, spacing;
};

struct ProbeSampleK {
    const float4* probes;
    const uint32_t* state;
    const float4* pos;
    const float4* nrm;
    float4* out;
    uint32_t* misses;
    uint32_t count;
    int dx, dy, dz;
    float ox, oy, oz, spacing;
};

// (c >> 1) << sh | (c & 1) << bit of coordinates c and c + 1 (vct_device.h texel_index_lg)
struct QAxis {
    uint32_t t0, t1;
    bool in0, in1;
};
__device__ __forceinline__ QAxis qaxis(int c, uint32_t nl, uint32_t sh, uint32_t bit) {
    const uint32_t u = (uint32_t)c, v = u + 1u;
    return QAxis{((u >> 1) << sh) | ((u & 1u) << bit), ((v >> 1) << sh) | ((v & 1u) << bit), u < nl, v < nl};
}

__device__ __forceinline__ float4 fma4(float w, float4 v, float4 acc) {
    return make_float4(fmaf(w, v.x, acc.x), fmaf(w, v.y, acc.y), fmaf(w, v.z, acc.z), fmaf(w, v.w, acc.w));
}

// S_l(q) for a wave-uniform level l; called under the exec mask of the lanes that sample it,
// whose q lies in [0, n]^3 (so the corner coordinates are in [-1, n_l])
__device__ __forceinline__ float4 sample_rgba(const QueryGrid& g, int l, float qx, float qy, float qz, int fx, int fy,
                                              int fz, float wdx, float wdy, float wdz) {
    const float scale = __uint_as_float((uint32_t)(127 - l) << 23);   // 2^-l, exact
    const float cx = qx * scale - 0.5f, cy = qy * scale - 0.5f, cz = qz * scale - 0.5f;
    const float flx = floorf(cx), fly = floorf(cy), flz = floorf(cz);
    const float ax = cx - flx, ay = cy - fly, az = cz - flz;
    const float wx[2] = {1.0f - ax, ax}, wy[2] = {1.0f - ay, ay}, wz[2] = {1.0f - az, az};
    const uint32_t lg = (uint32_t)(g.lgn - l), lnb = lg > 0u ? lg - 1u : 0u, nl = 1u << lg;
    const QAxis X = qaxis((int)flx, nl, 3u, 0u), Y = qaxis((int)fly, nl, lnb + 3u, 1u),
                Z = qaxis((int)flz, nl, 2u * lnb + 3u, 2u);
    const uint32_t xs[2] = {X.t0, X.t1}, ys[2] = {Y.t0, Y.t1}, zs[2] = {Z.t0, Z.t1};
    const bool ix[2] = {X.in0, X.in1}, iy[2] = {Y.in0, Y.in1}, iz[2] = {Z.in0, Z.in1};
    const bool faces = l != 0 && g.aniso;
    const uint32_t shf = 3u * lg;                                      // face f starts at texel f << shf
    const float4* const base = g.lvl[l];
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 acc = zero;
    if (!faces) {
        float4 v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bool in = ix[c & 1] && iy[(c >> 1) & 1] && iz[c >> 2];
            const uint32_t t = xs[c & 1] | ys[(c >> 1) & 1] | zs[c >> 2];
            v[c] = in ? base[(size_t)t] : zero;
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) acc = fma4((wx[c & 1] * wy[(c >> 1) & 1]) * wz[c >> 2], v[c], acc);
        return acc;
    }
    const uint32_t FX = (uint32_t)fx << shf, FY = (uint32_t)fy << shf, FZ = (uint32_t)fz << shf;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool in = ix[c & 1] && iy[(c >> 1) & 1] && iz[c >> 2];
        const uint32_t t = xs[c & 1] | ys[(c >> 1) & 1] | zs[c >> 2];
        float4 vx = zero, vy = zero, vz = zero;
        if (in) {
            vx = base[(size_t)(t | FX)];
            vy = base[(size_t)(t | FY)];
            vz = base[(size_t)(t | FZ)];
        }
        const float4 v = make_float4(fmaf(wdz, vz.x, fmaf(wdy, vy.x, wdx * vx.x)), fmaf(wdz, vz.y, fmaf(wdy, vy.y, wdx * vx.y)),
                                     fmaf(wdz, vz.z, fmaf(wdy, vy.z, wdx * vx.z)), fmaf(wdz, vz.w, fmaf(wdy, vy.w, wdx * vx.w)));
        acc = fma4((wx[c & 1] * wy[(c >> 1) & 1]) * wz[c >> 2], v, acc);
    }
    return acc;
}

// "cone queries": the march of one cone per lane, the wave together; o: the origin in voxel
// units, tau as given.  Returns (c.rgb, a); +0 and no step for a lane with need == false.
__device__ __forceinline__ float4 march_rgba(const QueryGrid& g, bool need, float ox, float oy, float oz, float dx,
                                             float dy, float dz, float tau_in, float t_lim, uint32_t& steps) {
    const float tau = fminf(fmaxf(tau_in, VCT_SPEC_TAU_MIN), VCT_SPEC_TAU_MAX);
    const float tau2 = 2.0f * tau;
    const float nf = (float)g.n, Lf = (float)g.L;
    const int fx = dx >= 0.0f ? VCT_FACE_PX : VCT_FACE_NX;
    const int fy = dy >= 0.0f ? VCT_FACE_PY : VCT_FACE_NY;
    const int fz = dz >= 0.0f ? VCT_FACE_PZ : VCT_FACE_NZ;
    const float wdx = dx * dx, wdy = dy * dy, wdz = dz * dz;
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // c.w is a
    float t = 1.0f;
    bool act = need;
    for (int it = 0; it < VCT_QUERY_MAX_STEPS; ++it) {
        // step 1
        const float qx = ox + dx * t, qy = oy + dy * t, qz = oz + dz * t;
        act = act & (c.w < VCT_ALPHA_STOP) & (t <= g.tmax) & !(t >= t_lim) &
              ((qx >= 0.0f) & (qx <= nf) & (qy >= 0.0f) & (qy <= nf) & (qz >= 0.0f) & (qz <= nf));
        const unsigned long long am = __builtin_amdgcn_ballot_w64(act);
        if (am == 0ull) break;
        // step 2, per lane (tau is clamped and t <= tmax on a marching lane: 0 <= m <= L)
        const float D = fmaxf(1.0f, tau2 * t);
        const float m = fminf(spec_log2(D), Lf);
        const int l0 = act ? (int)m : 0;
        const float fr = m - (float)l0;
        // step 3: one pass per level present among the marching lanes
        float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (unsigned long long pend = am; pend != 0ull;) {
            const int l = __builtin_amdgcn_readlane(l0, __builtin_ctzll(pend));
            const bool mine = act & (l0 == l);
            if (mine) s = sample_rgba(g, l, qx, qy, qz, fx, fy, fz, wdx, wdy, wdz);
            pend &= ~__builtin_amdgcn_ballot_w64(mine);
        }
        const bool two = act & (fr > 0.0f) & (l0 < g.L);
        float4 s1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (unsigned long long pend = __builtin_amdgcn_ballot_w64(two); pend != 0ull;) {
            const int l = __builtin_amdgcn_readlane(l0, __builtin_ctzll(pend));
            const bool mine = two & (l0 == l);
            if (mine) s1 = sample_rgba(g, l + 1, qx, qy, qz, fx, fy, fz, wdx, wdy, wdz);
            pend &= ~__builtin_amdgcn_ballot_w64(mine);
        }
        if (two) {
            const float omf = 1.0f - fr;
            s = make_float4(fmaf(fr, s1.x, omf * s.x), fmaf(fr, s1.y, omf * s.y), fmaf(fr, s1.z, omf * s.z),
                            fmaf(fr, s1.w, omf * s.w));
        }
        // steps 4, 5
        if (act) {
            c = fma4(1.0f - c.w, s, c);
            steps += 1u;
        }
        t = t + VCT_STEP_SCALE * D;
    }
    return c;
}

__global__ void __launch_bounds__(64) kquery(const QueryK k) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const bool in = i < k.count;
    const size_t r = in ? (size_t)i * 3u : 0u;
    const float4 a = k.cones[r], b = k.cones[r + 1], e = k.cones[r + 2];     // (p, tau) (d, t_lim) (off, valid)
    const bool need = in && e.w != 0.0f;
    const float ox = (a.x - k.g.g0x) * k.g.inv_h + e.x, oy = (a.y - k.g.g0y) * k.g.inv_h + e.y,
                oz = (a.z - k.g.g0z) * k.g.inv_h + e.z;
    uint32_t steps = 0;
    const float4 c = march_rgba(k.g, need, ox, oy, oz, b.x, b.y, b.z, a.w, b.w, steps);
    if (in) {
        k.out[i] = c;
        if (k.steps) k.steps[i] = steps;
    }
    if (k.steps_total) {
        const uint32_t ws = wave_sum_u32(steps);
        if (threadIdx.x == 0 && ws) atomicAdd(k.steps_total, (unsigned long long)ws);
    }
}

__global__ void __launch_bounds__(64) kprobe_build(const ProbeBuildK k) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const bool in = i < k.lanes;
    const uint32_t pr = in ? i / 6u : 0u, f = in ? i - pr * 6u : 0u;
    const uint32_t pz = pr / (k.dx * k.dy), rem = pr - pz * (k.dx * k.dy), py = rem / k.dx, px = rem - py * k.dx;
    const float Px = fmaf((float)px, k.spacing, k.ox), Py = fmaf((float)py, k.spacing, k.oy),
                Pz = fmaf((float)pz, k.spacing, k.oz);
    // the cone record's origin with off = +0 (kquery's expression)
    const float ox = (Px - k.g.g0x) * k.g.inv_h + 0.0f, oy = (Py - k.g.g0y) * k.g.inv_h + 0.0f,
                oz = (Pz - k.g.g0z) * k.g.inv_h + 0.0f;
    const float sgn = (f & 1u) ? -1.0f : 1.0f;
    const float dx = (f >> 1) == 0u ? sgn : 0.0f, dy = (f >> 1) == 1u ? sgn : 0.0f, dz = (f >> 1) == 2u ? sgn : 0.0f;
    uint32_t steps = 0;
    const float4 c = march_rgba(k.g, in, ox, oy, oz, dx, dy, dz, VCT_SPEC_TAU_MAX, __builtin_inff(), steps);
    if (in) {
        k.probes[i] = c;
        if (f == 0u) {
            const float nf = (float)k.g.n;
            uint32_t st = 0u;
            if ((ox >= 0.0f) & (ox < nf) & (oy >= 0.0f) & (oy < nf) & (oz >= 0.0f) & (oz < nf))
                st = occ_at(k.occ_bits, k.g.n, (int)floorf(ox), (int)floorf(oy), (int)floorf(oz)) ? 0u : 1u;
            k.state[pr] = st;
        }
    }
    if (k.steps_total) {
        const uint32_t ws = wave_sum_u32(steps);
        if (threadIdx.x == 0 && ws) atomicAdd(k.steps_total, (unsigned long long)ws);
    }
}

// one axis of "probe grid", sample: the lower corner and the two weights
__device__ __forceinline__ void probe_axis(float p, float origin, float spacing, int dim, int& i0, float w[2]) {
    float g = (p - origin) / spacing;
    g = fminf(fmaxf(g, 0.0f), (float)(dim - 1));
    i0 = dim == 1 ? 0 : min((int)floorf(g), dim - 2);
    const float fr = g - (float)i0;
    w[0] = 1.0f - fr;
    w[1] = fr;
}

__global__ void __launch_bounds__(64) kprobe_sample(const ProbeSampleK k) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const bool in = i < k.count;
    uint32_t miss = 0u;
    if (in) {
        const float4 P = k.pos[i];
        float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (P.w != 0.0f) {
            const float4 N = k.nrm[i];
            int ix, iy, iz;
            float wx[2], wy[2], wz[2];
            probe_axis(P.x, k.ox, k.spacing, k.dx, ix, wx);
            probe_axis(P.y, k.oy, k.spacing, k.dy, iy, wy);
            probe_axis(P.z, k.oz, k.spacing, k.dz, iz, wz);
            const int fx = N.x >= 0.0f ? VCT_FACE_PX : VCT_FACE_NX;
            const int fy = N.y >= 0.0f ? VCT_FACE_PY : VCT_FACE_NY;
            const int fz = N.z >= 0.0f ? VCT_FACE_PZ : VCT_FACE_NZ;
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float4 Sx = zero, Sy = zero, Sz = zero;
            float W = 0.0f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int x = ix + (c & 1), y = iy + ((c >> 1) & 1), z = iz + (c >> 2);
                if (x >= k.dx || y >= k.dy || z >= k.dz) continue;
                const size_t pr = ((size_t)z * (size_t)k.dy + (size_t)y) * (size_t)k.dx + (size_t)x;
                if (k.state[pr] == 0u) continue;
                const float wc = (wx[c & 1] * wy[(c >> 1) & 1]) * wz[c >> 2];
                W = W + wc;
                Sx = fma4(wc, k.probes[pr * 6u + (size_t)fx], Sx);
                Sy = fma4(wc, k.probes[pr * 6u + (size_t)fy], Sy);
                Sz = fma4(wc, k.probes[pr * 6u + (size_t)fz], Sz);
            }
            const float wnx = N.x * N.x, wny = N.y * N.y, wnz = N.z * N.z;
            const float4 V = make_float4(fmaf(wnz, Sz.x, fmaf(wny, Sy.x, wnx * Sx.x)), fmaf(wnz, Sz.y, fmaf(wny, Sy.y, wnx * Sx.y)),
                                         fmaf(wnz, Sz.z, fmaf(wny, Sy.z, wnx * Sx.z)), fmaf(wnz, Sz.w, fmaf(wny, Sy.w, wnx * Sx.w)));
            if (W > 0.0f) {
                out = make_float4(V.x / W, V.y / W, V.z / W, 1.0f - V.w / W);
            } else {
                out = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
                miss = 1u;
            }
        }
        k.out[i] = out;
    }
    if (k.misses) {
        const uint32_t ws = wave_sum_u32(miss);
        if (threadIdx.x == 0 && ws) atomicAdd(k.misses, ws);
    }
}

// ---- host side --------------------------------------------------------------------------
void query_grid(const Grid& g, QueryGrid& q) {
    for (int i = 0; i <= (int)g.L; ++i) q.lvl[i] = g.pyr + g.lvl_off[i];
    q.n = (int)g.n; q.L = (int)g.L; q.lgn = __builtin_ctz(g.n); q.aniso = g.aniso;
    q.g0x = g.g0[0]; q.g0y = g.g0[1]; q.g0z = g.g0[2]; q.inv_h = g.inv_h;
    q.tmax = (float)g.n * VCT_SQRT3;
}

// the input rule of "probe grid"; nullptr, or what is wrong
const char* check_probe_grid(const vct_probe_grid* pg) {
    if (!pg) return "NULL grid";
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(pg->origin[k])) return "non-finite origin";
        if (pg->dims[k] < 1u || pg->dims[k] > (uint32_t)VCT_PROBE_MAX_DIM) return "dims outside 1 .. VCT_PROBE_MAX_DIM";
    }
    if (!std::isfinite(pg->spacing) || !(pg->spacing > 0.0f)) return "spacing not finite or not > 0";
    return nullptr;
}

}  // namespace
}  // namespace vct

using namespace vct;

extern "C" vct_status vct_cone_query_device(vct_ctx* c, const vct_cone_query_args* a) {
    if (!c) return VCT_EINVAL;
    if (!a) return lfail(c, VCT_EINVAL, "cone_query: NULL args");
    if (!a->cones || !a->out4) return lfail(c, VCT_EINVAL, "cone_query: NULL cones or out4");
    if ((((uintptr_t)a->cones | (uintptr_t)a->out4) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "cone_query: cones and out4 must be 16-byte aligned");
    if (((uintptr_t)a->steps & 3u) != 0) return lfail(c, VCT_EINVAL, "cone_query: steps must be 4-byte aligned");
    if (((uintptr_t)a->cone_steps & 7u) != 0) return lfail(c, VCT_EINVAL, "cone_query: cone_steps must be 8-byte aligned");
    const Grid& g = c->grid;
    if (!g.voxelized || !g.mipped) return lfail(c, VCT_ESTATE, "cone_query before voxelize / build_mips");
    if (a->count == 0) return VCT_OK;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    QueryK k;
    std::memset(&k, 0, sizeof k);
    query_grid(g, k.g);
    k.cones = (const float4*)a->cones; k.out = (float4*)a->out4; k.steps = a->steps; k.steps_total = a->cone_steps;
    k.count = a->count;
    hipLaunchKernelGGL(kquery, dim3((a->count + 63u) / 64u), dim3(64), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "cone_query");
    return VCT_OK;
}

extern "C" vct_status vct_probe_build_device(vct_ctx* c, const vct_probe_grid* pg, float* probes, uint32_t* state,
                                             unsigned long long* cone_steps) {
    if (!c) return VCT_EINVAL;
    if (const char* bad = check_probe_grid(pg)) return lfail(c, VCT_EINVAL, std::string("probe_build: ") + bad);
    if (!probes || !state) return lfail(c, VCT_EINVAL, "probe_build: NULL probes or state");
    if (((uintptr_t)probes & 15u) != 0) return lfail(c, VCT_EINVAL, "probe_build: probes must be 16-byte aligned");
    if (((uintptr_t)state & 3u) != 0) return lfail(c, VCT_EINVAL, "probe_build: state must be 4-byte aligned");
    if (((uintptr_t)cone_steps & 7u) != 0) return lfail(c, VCT_EINVAL, "probe_build: cone_steps must be 8-byte aligned");
    const Grid& g = c->grid;
    if (!g.voxelized || !g.mipped) return lfail(c, VCT_ESTATE, "probe_build before voxelize / build_mips");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    ProbeBuildK k;
    std::memset(&k, 0, sizeof k);
    query_grid(g, k.g);
    k.occ_bits = g.occ_bits; k.probes = (float4*)probes; k.state = state; k.steps_total = cone_steps;
    k.dx = pg->dims[0]; k.dy = pg->dims[1]; k.dz = pg->dims[2];
    k.lanes = 6u * k.dx * k.dy * k.dz;                       // <= 6 * 256^3 < 2^32
    k.ox = pg->origin[0]; k.oy = pg->origin[1]; k.oz = pg->origin[2]; k.spacing = pg->spacing;
    hipLaunchKernelGGL(kprobe_build, dim3((k.lanes + 63u) / 64u), dim3(64), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "probe_build");
    return VCT_OK;
}

extern "C" vct_status vct_probe_sample_device(vct_ctx* c, const vct_probe_grid* pg, const float* probes,
                                              const uint32_t* state, const float* pos4, const float* nrm4,
                                              uint32_t count, float* out4, uint32_t* misses) {
    if (!c) return VCT_EINVAL;
    if (const char* bad = check_probe_grid(pg)) return lfail(c, VCT_EINVAL, std::string("probe_sample: ") + bad);
    if (!probes || !state || !pos4 || !nrm4 || !out4) return lfail(c, VCT_EINVAL, "probe_sample: NULL buffer");
    if ((((uintptr_t)probes | (uintptr_t)pos4 | (uintptr_t)nrm4 | (uintptr_t)out4) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "probe_sample: float4 buffers must be 16-byte aligned");
    if ((((uintptr_t)state | (uintptr_t)misses) & 3u) != 0)
        return lfail(c, VCT_EINVAL, "probe_sample: state and misses must be 4-byte aligned");
    if (count == 0) return VCT_OK;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    ProbeSampleK k;
    std::memset(&k, 0, sizeof k);
    k.probes = (const float4*)probes; k.state = state; k.pos = (const float4*)pos4; k.nrm = (const float4*)nrm4;
    k.out = (float4*)out4; k.misses = misses; k.count = count;
    k.dx = (int)pg->dims[0]; k.dy = (int)pg->dims[1]; k.dz = (int)pg->dims[2];
    k.ox = pg->origin[0]; k.oy = pg->origin[1]; k.oz = pg->origin[2]; k.spacing = pg->spacing;
    hipLaunchKernelGGL(kprobe_sample, dim3((count + 63u) / 64u), dim3(64), 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "probe_sample");
    return VCT_OK;
}
