// vct_voxview.hip — the voxel view and ray picking (include/vct_voxview.h; the arithmetic is
// include/vct_spec.h "voxel view").
//
//   walk_cells   the one device function: a ray (origin in level-0 voxel units, direction as
//                given, limit) is normalised by the K2 direction rule, clipped to the level's
//                grid by the fog march's slab, and walked cell by cell (A.3's walk, as
//                dda_visibility of vct_device.h writes it) until the first solid cell, the grid's
//                edge or the limit.  The cell is tested first, then stepped.  Solid is K1's
//                occupancy bit, or alpha > 0 in any face of the level's texel: while walking only
//                the .w dwords are loaded.
//   kvox_pick    one ray per lane, in list order, rays from memory.
//   kvox_view    one pixel per lane, 8 x 8 pixels per wave (K4's screen tiling, so a wave's rays
//                stay in neighbouring cells), rays generated in registers from the camera record
//                (camera_fields / pixel_ray of vct_view.h); the hit cell's float4 is loaded once,
//                after the walk.  Because both kernels call walk_cells, the view's records equal the
//                pick's on the same rays in every bit.
//
// The level is uniform per launch: its base pointer, size and shifts are kernel arguments
// (scalar registers).  Texel addresses are texel_index_lg of the brick layout, 64-bit from the
// level's base (a 1024^3 anisotropic level is past a 32-bit buffer range).  Every cell read lies
// in [0, n_l)^3: the start cell is clamped as a float before the conversion, and a step that
// leaves the range ends the walk before anything is read.  No lane reads another lane's ray, and
// the only atomic is the wave-summed counter of tested cells.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "vct_internal.h"
#include "vct_view.h"

namespace vct {
namespace {

struct VoxLevel {
    const float4* lvl;                       // texel 0 of the level (face 0)
    const float4* albedo_occ;                // K1's [n^3] records, linear-Z
    const float4* normal;
    const unsigned long long* occ_bits;
    int nl, lg, faces;                       // n_l = 1 << lg cells per axis; faces: six face volumes
    float g0x, g0y, g0z, inv_h;
    float down, up;                          // 2^-l and 2^l
};

struct PickK {
    VoxLevel g;
    const float4* org;
    const float4* dir;
    uint4* hit;
    unsigned long long* cells;
    uint32_t count;
};

struct ViewK {
    VoxLevel g;
    int w, h;
    float fx, fy, fz, ux, uy, uz, rx, ry, rz, tan_half, aspect;   // camera_fields
    float ox, oy, oz;                        // the eye in level-0 voxel units
    float4* lin;
    uint32_t* rgba8;
    uint4* hit;
    unsigned long long* cells;
    int mode, shade;
};

struct VoxHit {
    uint32_t cell, face, steps;
    float t;
    float dx, dy, dz;                        // the normalised direction (the view's face blend)
    int x, y, z;                             // the hit cell
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }

template <bool kAlpha>
__device__ __forceinline__ bool cell_solid(const VoxLevel& g, int x, int y, int z) {
    if (!kAlpha) return occ_at(g.occ_bits, g.nl, x, y, z);
    const size_t t = texel_index_lg((uint32_t)x, (uint32_t)y, (uint32_t)z, (uint32_t)g.lg);
    const float* const a = (const float*)g.lvl + 3;          // the .w dword of texel 0
    bool s = a[t * 4u] > 0.0f;
    if (g.faces) {
        const uint32_t shf = 3u * (uint32_t)g.lg;            // face f starts at texel f << shf
#pragma unroll
        for (uint32_t f = 1; f < (uint32_t)VCT_NUM_FACES; ++f) s |= a[(t + ((size_t)f << shf)) * 4u] > 0.0f;
    }
    return s;
}

// one axis of the slab: clips [t0, t1] (a0 = c when it raises t0) or, where it does not clip,
// keeps `ok` only with the origin between its planes
__device__ __forceinline__ void slab_axis(float o, float d, float nf, int c, float& t0, float& t1, int& a0, bool& ok) {
    const float inv = 1.0f / d;
    if (d != 0.0f && finite_f(inv)) {
        const float ta = (0.0f - o) * inv, tb = (nf - o) * inv;
        const float tn = fminf(ta, tb), tf = fmaxf(ta, tb);
        if (tn > t0) { t0 = tn; a0 = c; }
        t1 = fminf(t1, tf);
    } else {
        ok = ok && o >= 0.0f && o <= nf;
    }
}

// "voxel view": the walk of one ray.  o: the origin in level-0 voxel units; v: the direction as
// given.  A lane with need == false walks nothing and reads nothing.
template <bool kAlpha>
__device__ __forceinline__ VoxHit walk_cells(const VoxLevel& g, bool need, float ox, float oy, float oz, float vx,
                                             float vy, float vz, float t_lim) {
    const float inf = __builtin_inff();
    const float len = sqrtf(dot3(vx, vy, vz, vx, vy, vz));
    const float dx = vx / len, dy = vy / len, dz = vz / len;
    VoxHit h{VCT_VOXHIT_CELL_MISS, VCT_VOXHIT_FACE_MISS, 0u, inf, dx, dy, dz, 0, 0, 0};
    const float ll = (t_lim != t_lim ? inf : t_lim) * g.down;
    const float olx = ox * g.down, oly = oy * g.down, olz = oz * g.down;
    bool ok = need && len > 0.0f && finite_f(len) && finite_f(ox) && finite_f(oy) && finite_f(oz) && finite_f(dx) &&
              finite_f(dy) && finite_f(dz);
    // slab
    const float nf = (float)g.nl;
    float t0 = 0.0f, t1 = ll;
    int a0 = -1;
    slab_axis(olx, dx, nf, 0, t0, t1, a0, ok);
    slab_axis(oly, dy, nf, 1, t0, t1, a0, ok);
    slab_axis(olz, dz, nf, 2, t0, t1, a0, ok);
    ok = ok && ll > 0.0f && t1 > t0;
    if (!ok) return h;
    // walk
    int sx = dx > 0.0f ? 1 : (dx < 0.0f ? -1 : 0);
    int sy = dy > 0.0f ? 1 : (dy < 0.0f ? -1 : 0);
    int sz = dz > 0.0f ? 1 : (dz < 0.0f ? -1 : 0);
    const float tdx = sx ? 1.0f / fabsf(dx) : inf;
    const float tdy = sy ? 1.0f / fabsf(dy) : inf;
    const float tdz = sz ? 1.0f / fabsf(dz) : inf;
    if (tdx == inf) sx = 0;
    if (tdy == inf) sy = 0;
    if (tdz == inf) sz = 0;
    const float px = olx + dx * t0, py = oly + dy * t0, pz = olz + dz * t0;
    int x = (int)fminf(fmaxf(floorf(px), 0.0f), nf - 1.0f);
    int y = (int)fminf(fmaxf(floorf(py), 0.0f), nf - 1.0f);
    int z = (int)fminf(fmaxf(floorf(pz), 0.0f), nf - 1.0f);
    float tmx = sx > 0 ? ((float)(x + 1) - px) * tdx : (sx < 0 ? (px - (float)x) * tdx : inf);
    float tmy = sy > 0 ? ((float)(y + 1) - py) * tdy : (sy < 0 ? (py - (float)y) * tdy : inf);
    float tmz = sz > 0 ? ((float)(z + 1) - pz) * tdz : (sz < 0 ? (pz - (float)z) * tdz : inf);
    uint32_t face = VCT_VOXHIT_FACE_INSIDE;
    if (a0 == 0) face = sx > 0 ? 0u : 1u;
    if (a0 == 1) face = sy > 0 ? 2u : 3u;
    if (a0 == 2) face = sz > 0 ? 4u : 5u;
    float te = t0;
    const int cap = VCT_VOXVIEW_STEPS_PER_CELL * g.nl;
    for (int it = 0; it < cap; ++it) {
        h.steps += 1u;
        if (cell_solid<kAlpha>(g, x, y, z)) {
            h.cell = (uint32_t)x + (uint32_t)g.nl * ((uint32_t)y + (uint32_t)g.nl * (uint32_t)z);
            h.face = face;
            h.t = te * g.up;
            h.x = x; h.y = y; h.z = z;
            break;
        }
        if (tmx <= tmy && tmx <= tmz) {
            const float tn = t0 + tmx;
            if (tn >= ll) break;
            x += sx;
            if (x < 0 || x >= g.nl) break;
            tmx = tmx + tdx; face = sx > 0 ? 0u : 1u; te = tn;
        } else if (tmy <= tmz) {
            const float tn = t0 + tmy;
            if (tn >= ll) break;
            y += sy;
            if (y < 0 || y >= g.nl) break;
            tmy = tmy + tdy; face = sy > 0 ? 2u : 3u; te = tn;
        } else {
            const float tn = t0 + tmz;
            if (tn >= ll) break;
            z += sz;
            if (z < 0 || z >= g.nl) break;
            tmz = tmz + tdz; face = sz > 0 ? 4u : 5u; te = tn;
        }
    }
    return h;
}

__device__ __forceinline__ uint4 hit_record(const VoxHit& h) {
    return make_uint4(h.cell, h.face, h.steps, __float_as_uint(h.t));
}

__device__ __forceinline__ void add_cells(unsigned long long* cells, uint32_t steps) {
    if (cells) {
        const uint32_t ws = wave_sum_u32(steps);
        if (threadIdx.x == 0 && ws) atomicAdd(cells, (unsigned long long)ws);
    }
}

template <bool kAlpha>
__global__ void __launch_bounds__(64) kvox_pick(const PickK k) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const bool in = i < k.count;
    const size_t r = in ? (size_t)i : 0u;
    const float4 o = k.org[r], d = k.dir[r];
    const float ox = (o.x - k.g.g0x) * k.g.inv_h, oy = (o.y - k.g.g0y) * k.g.inv_h, oz = (o.z - k.g.g0z) * k.g.inv_h;
    const VoxHit h = walk_cells<kAlpha>(k.g, in, ox, oy, oz, d.x, d.y, d.z, d.w);
    if (in) k.hit[i] = hit_record(h);
    add_cells(k.cells, h.steps);
}

// the colour of the hit cell by mode ("voxel view", Colour), before the shade
__device__ __forceinline__ void hit_colour(const VoxLevel& g, int mode, const VoxHit& h, float& r, float& gg, float& b) {
    if (mode == VCT_VOXVIEW_ALBEDO) {
        const float4 a = g.albedo_occ[(size_t)h.cell];
        r = a.x; gg = a.y; b = a.z;
        return;
    }
    if (mode == VCT_VOXVIEW_NORMAL) {
        const float4 n = g.normal[(size_t)h.cell];
        r = fmaf(0.5f, n.x, 0.5f); gg = fmaf(0.5f, n.y, 0.5f); b = fmaf(0.5f, n.z, 0.5f);
        return;
    }
    const size_t t = texel_index_lg((uint32_t)h.x, (uint32_t)h.y, (uint32_t)h.z, (uint32_t)g.lg);
    float4 T;
    if (!g.faces) {
        T = g.lvl[t];
    } else {
        const uint32_t shf = 3u * (uint32_t)g.lg;
        const size_t fx = h.dx >= 0.0f ? VCT_FACE_PX : VCT_FACE_NX;
        const size_t fy = h.dy >= 0.0f ? VCT_FACE_PY : VCT_FACE_NY;
        const size_t fz = h.dz >= 0.0f ? VCT_FACE_PZ : VCT_FACE_NZ;
        const float wdx = h.dx * h.dx, wdy = h.dy * h.dy, wdz = h.dz * h.dz;
        const float4 X = g.lvl[t + (fx << shf)], Y = g.lvl[t + (fy << shf)], Z = g.lvl[t + (fz << shf)];
        T = make_float4(fmaf(wdz, Z.x, fmaf(wdy, Y.x, wdx * X.x)), fmaf(wdz, Z.y, fmaf(wdy, Y.y, wdx * X.y)),
                        fmaf(wdz, Z.z, fmaf(wdy, Y.z, wdx * X.z)), fmaf(wdz, Z.w, fmaf(wdy, Y.w, wdx * X.w)));
    }
    if (mode == VCT_VOXVIEW_ALPHA) { r = T.w; gg = T.w; b = T.w; }
    else { r = T.x; gg = T.y; b = T.z; }
}

template <bool kAlpha>
__global__ void __launch_bounds__(64) kvox_view(const ViewK k) {
    // lane -> pixel of the wave's 8 x 8 tile
    const int x = (int)blockIdx.x * 8 + (int)(threadIdx.x & 7u), y = (int)blockIdx.y * 8 + (int)(threadIdx.x >> 3);
    const bool in = x < k.w && y < k.h;
    float vx, vy, vz;
    pixel_ray(k, x, y, vx, vy, vz);
    const VoxHit h = walk_cells<kAlpha>(k.g, in, k.ox, k.oy, k.oz, vx, vy, vz, __builtin_inff());
    if (in) {
        const size_t p = (size_t)y * (size_t)k.w + (size_t)x;
        float4 lin = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        uint32_t q = 0u;
        if (h.cell != VCT_VOXHIT_CELL_MISS) {
            float r, g, b;
            hit_colour(k.g, k.mode, h, r, g, b);
            if (k.shade) {
                const uint32_t ax = h.face >> 1;
                const float s = ax == 0u ? VCT_VOXVIEW_SHADE_X
                                         : (ax == 1u ? VCT_VOXVIEW_SHADE_Y : (ax == 2u ? VCT_VOXVIEW_SHADE_Z : 1.0f));
                r = r * s; g = g * s; b = b * s;
            }
            lin = make_float4(r, g, b, 1.0f);
            if (k.rgba8)
                q = k.mode == VCT_VOXVIEW_RADIANCE ? (to8(r) | (to8(g) << 8) | (to8(b) << 16) | 0xff000000u)
                                                   : (quant8(r) | (quant8(g) << 8) | (quant8(b) << 16) | 0xff000000u);
        }
        if (k.lin) k.lin[p] = lin;
        if (k.rgba8) k.rgba8[p] = q;
        if (k.hit) k.hit[p] = hit_record(h);
    }
    add_cells(k.cells, h.steps);
}

// ---- host side --------------------------------------------------------------------------
void vox_level(const Grid& g, uint32_t level, VoxLevel& v) {
    v.lvl = g.pyr + g.lvl_off[level];
    v.albedo_occ = g.albedo_occ; v.normal = g.normal; v.occ_bits = g.occ_bits;
    v.lg = (int)__builtin_ctz(g.n) - (int)level;
    v.nl = 1 << v.lg;
    v.faces = level != 0 && g.aniso;
    v.g0x = g.g0[0]; v.g0y = g.g0[1]; v.g0z = g.g0[2]; v.inv_h = g.inv_h;
    v.down = ldexpf(1.0f, -(int)level);
    v.up = ldexpf(1.0f, (int)level);
}

// the level / solid-source rule the two calls share; nullptr, or what is wrong (*st its status)
const char* check_source(const Grid& g, uint32_t level, bool alpha, vct_status* st) {
    *st = VCT_EINVAL;
    if (level > g.L) return "level above L";
    if (!alpha && level != 0) return "K1's occupancy, albedo and normal exist at level 0 only";
    *st = VCT_ESTATE;
    if (!alpha && !g.voxelized) return "before voxelize";
    if (alpha && level == 0 && !(g.injected || g.mipped)) return "level 0 before an inject or upload";
    if (alpha && level != 0 && !g.mipped) return "a level >= 1 before build_mips";
    return nullptr;
}

}  // namespace
}  // namespace vct

using namespace vct;

extern "C" vct_status vct_voxel_pick_device(vct_ctx* c, const vct_voxel_pick_args* a) {
    if (!c) return VCT_EINVAL;
    if (!a) return lfail(c, VCT_EINVAL, "voxel_pick: NULL args");
    if (!a->org4 || !a->dir4 || !a->hit4) return lfail(c, VCT_EINVAL, "voxel_pick: NULL org4, dir4 or hit4");
    if ((((uintptr_t)a->org4 | (uintptr_t)a->dir4 | (uintptr_t)a->hit4) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "voxel_pick: org4, dir4 and hit4 must be 16-byte aligned");
    if (((uintptr_t)a->cells & 7u) != 0) return lfail(c, VCT_EINVAL, "voxel_pick: cells must be 8-byte aligned");
    if (a->solid != VCT_VOXPICK_OCCUPANCY && a->solid != VCT_VOXPICK_ALPHA)
        return lfail(c, VCT_EINVAL, "voxel_pick: solid outside VCT_VOXPICK_*");
    const bool alpha = a->solid == VCT_VOXPICK_ALPHA;
    const Grid& g = c->grid;
    vct_status st;
    if (const char* bad = check_source(g, a->level, alpha, &st)) return lfail(c, st, std::string("voxel_pick: ") + bad);
    if (a->count == 0) return VCT_OK;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    PickK k;
    std::memset(&k, 0, sizeof k);
    vox_level(g, a->level, k.g);
    k.org = (const float4*)a->org4; k.dir = (const float4*)a->dir4; k.hit = (uint4*)a->hit4; k.cells = a->cells;
    k.count = a->count;
    const dim3 grid((a->count + 63u) / 64u), block(64);
    if (alpha) hipLaunchKernelGGL(kvox_pick<true>, grid, block, 0, c->stream, k);
    else hipLaunchKernelGGL(kvox_pick<false>, grid, block, 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "voxel_pick");
    return VCT_OK;
}

extern "C" vct_status vct_voxel_view_device(vct_ctx* c, const vct_camera* cam, const vct_voxel_view_args* a) {
    if (!c) return VCT_EINVAL;
    if (!cam || !a) return lfail(c, VCT_EINVAL, "voxel_view: NULL camera or args");
    if (const char* bad = gbuffer_input_error(cam, a->width, a->height))
        return lfail(c, VCT_EINVAL, std::string("voxel_view: ") + bad);
    if (!a->linear4 && !a->rgba8 && !a->hit4) return lfail(c, VCT_EINVAL, "voxel_view: no output");
    if ((((uintptr_t)a->linear4 | (uintptr_t)a->hit4) & 15u) != 0)
        return lfail(c, VCT_EINVAL, "voxel_view: linear4 and hit4 must be 16-byte aligned");
    if (((uintptr_t)a->rgba8 & 3u) != 0) return lfail(c, VCT_EINVAL, "voxel_view: rgba8 must be 4-byte aligned");
    if (((uintptr_t)a->cells & 7u) != 0) return lfail(c, VCT_EINVAL, "voxel_view: cells must be 8-byte aligned");
    if (a->mode > (uint32_t)VCT_VOXVIEW_NORMAL) return lfail(c, VCT_EINVAL, "voxel_view: mode outside VCT_VOXVIEW_*");
    const bool alpha = a->mode == VCT_VOXVIEW_RADIANCE || a->mode == VCT_VOXVIEW_ALPHA;
    const Grid& g = c->grid;
    vct_status st;
    if (const char* bad = check_source(g, a->level, alpha, &st)) return lfail(c, st, std::string("voxel_view: ") + bad);
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    ViewK k;
    std::memset(&k, 0, sizeof k);
    vox_level(g, a->level, k.g);
    camera_fields(k, cam, a->width, a->height);
    k.ox = (cam->position[0] - g.g0[0]) * g.inv_h;
    k.oy = (cam->position[1] - g.g0[1]) * g.inv_h;
    k.oz = (cam->position[2] - g.g0[2]) * g.inv_h;
    k.lin = (float4*)a->linear4; k.rgba8 = a->rgba8; k.hit = (uint4*)a->hit4; k.cells = a->cells;
    k.mode = (int)a->mode; k.shade = a->shade != 0;
    const dim3 grid((a->width + 7u) / 8u, (a->height + 7u) / 8u), block(64);
    if (alpha) hipLaunchKernelGGL(kvox_view<true>, grid, block, 0, c->stream, k);
    else hipLaunchKernelGGL(kvox_view<false>, grid, block, 0, c->stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "voxel_view");
    return VCT_OK;
}
