// vct_bounce.hip — light bounces: cone-traced irradiance re-injected per voxel
// (include/vct_spec.h "light bounces", include/vct_bounce.h).
//
// The occupied voxels with a nonzero normal are the cone origins of one more K4 launch.
// They are kept as a materialised G-buffer (Bounce in vct_internal.h) rather than read
// from the voxel grids by a loader inside K4: the cone trace then runs the kernels it
// runs for a frame, unchanged, and the record (P = g0 + (x + 0.5) * hh, rounded to
// float) is the one the spec defines the gather on, so both ways give the same bits.
// The cost is 32 bytes of G-buffer per source, written once per voxelization.
//
//   k_bounce_regions   sources per 16^3 region (count pass), then, after k_bounce_scan,
//                      their records region by region, Morton order inside a region
//   k_bounce_list      the same records in occ_list order (A/B of the source order)
//   k_bounce_save      the level 0 the bounces add to, one texel per source
//   k_bounce_add       level 0 = L0 + A * I at every source (bricked level-0 layout)
#include <hip/hip_runtime.h>
#include "vct_internal.h"

namespace vct {
namespace {

// The frame pixel of source s: lane s % 64 of K4's unit s / 64 (k4_trace: unit -> 16x16
// block and 8x8 quarter of a 64x64 tile, lanes in Morton order), tiles row-major.
__host__ __device__ __forceinline__ uint32_t bounce_pixel(uint32_t s, uint32_t tiles_x) {
    const uint32_t lane = s & 63u, unit = s >> 6;
    const uint32_t wave = unit & 3u, rb = unit >> 2, sub = rb & 15u, lt = rb >> 4;
    const uint32_t mx = (lane & 1u) | ((lane >> 1) & 2u) | ((lane >> 2) & 4u);
    const uint32_t my = ((lane >> 1) & 1u) | ((lane >> 2) & 2u) | ((lane >> 3) & 4u);
    const uint32_t x = (lt % tiles_x) * VCT_TILE + (sub & 3u) * 16u + (wave & 1u) * 8u + mx;
    const uint32_t y = (lt / tiles_x) * VCT_TILE + (sub >> 2) * 16u + (wave >> 1) * 8u + my;
    return y * (tiles_x * VCT_TILE) + x;
}

struct SourceK {
    const unsigned long long* occ_bits;
    const float4* normal;
    uint32_t n;
    float g0x, g0y, g0z, hh;         // hh = E / (float)n
    uint32_t tiles_x;
    uint32_t* vox;
    float4* pos;
    float4* nrm;
};

// the G-buffer record of the source at voxel v = (x, y, z), written as source s
__device__ __forceinline__ void write_source(const SourceK& k, uint32_t s, uint32_t v, uint32_t x, uint32_t y,
                                             uint32_t z, float4 N) {
    const uint32_t pix = bounce_pixel(s, k.tiles_x);
    const float px = k.g0x + ((float)x + 0.5f) * k.hh;     // multiply, then add (-ffp-contract=off)
    const float py = k.g0y + ((float)y + 0.5f) * k.hh;
    const float pz = k.g0z + ((float)z + 0.5f) * k.hh;
    k.vox[s] = v;
    k.pos[pix] = make_float4(px, py, pz, 1.0f);
    k.nrm[pix] = make_float4(N.x, N.y, N.z, 0.0f);
}

__device__ __forceinline__ bool is_source(float4 N) { return N.x != 0.0f || N.y != 0.0f || N.z != 0.0f; }

// bits 0, 3, 6, 9 of v -> bits 0..3 (one axis of a 12-bit Morton index)
__device__ __forceinline__ uint32_t compact3(uint32_t v) {
    v &= 0x249u;
    v = (v | (v >> 2)) & 0x0c3u;
    v = (v | (v >> 4)) & 0x00fu;
    return v;
}

// inclusive sum over the block's threads (blockDim.x = T, a power of two)
template <int T>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* sh) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < (uint32_t)T; d <<= 1) {
        const uint32_t a = t >= d ? sh[t - d] : 0u;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    return sh[t];
}

// One block per region of R^3 voxels (R = min(16, n)); thread t takes the region's voxels
// with Morton indices [t * per, (t + 1) * per).  off == null: the count pass, cnt[region] =
// its sources.  Else the sources are written from off[region] on, in Morton order.
__global__ void __launch_bounds__(256) k_bounce_regions(SourceK k, uint32_t R, const uint32_t* __restrict__ off,
                                                        uint32_t* __restrict__ cnt) {
    __shared__ uint32_t sh[256];
    const uint32_t nr = k.n / R, r = blockIdx.x;
    const uint32_t bx = (r % nr) * R, by = ((r / nr) % nr) * R, bz = (r / (nr * nr)) * R;
    const uint32_t R3 = R * R * R, per = R3 >= 256u ? R3 / 256u : 1u;
    const uint32_t first = threadIdx.x * per;
    uint32_t m = 0;
    if (first < R3)
        for (uint32_t j = 0; j < per; ++j) {
            const uint32_t i = first + j;
            const uint32_t x = bx + compact3(i), y = by + compact3(i >> 1), z = bz + compact3(i >> 2);
            const uint32_t v = x + k.n * (y + k.n * z);
            if (((k.occ_bits[v >> 6] >> (v & 63u)) & 1ull) && is_source(k.normal[v])) m |= 1u << j;
        }
    const uint32_t mine = (uint32_t)__popc(m);
    const uint32_t incl = block_scan<256>(mine, sh);
    if (!off) {
        if (threadIdx.x == 255u) cnt[r] = incl;
        return;
    }
    uint32_t s = off[r] + incl - mine;
    for (uint32_t j = 0; j < per; ++j) {
        if (!((m >> j) & 1u)) continue;
        const uint32_t i = first + j;
        const uint32_t x = bx + compact3(i), y = by + compact3(i >> 1), z = bz + compact3(i >> 2);
        const uint32_t v = x + k.n * (y + k.n * z);
        write_source(k, s++, v, x, y, z, k.normal[v]);
    }
}

// a[0..cnt) -> its exclusive prefix sums, a[cnt] = the total (one block)
__global__ void __launch_bounds__(1024) k_bounce_scan(uint32_t* __restrict__ a, uint32_t cnt) {
    __shared__ uint32_t sh[1024];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < cnt; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < cnt ? a[i] : 0u;
        const uint32_t incl = block_scan<1024>(v, sh);
        if (i < cnt) a[i] = carry + incl - v;
        carry += sh[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) a[cnt] = carry;
}

// occ_list order (A/B): wave w of the launch appends the sources among its 64 list entries
// at *total, so the list keeps K1's order up to the order the waves arrive in
__global__ void __launch_bounds__(256) k_bounce_list(SourceK k, const uint32_t* __restrict__ occ_list,
                                                     const uint32_t* __restrict__ occ_count, uint32_t* total) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t v = 0;
    float4 N = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i < *occ_count) {
        v = occ_list[i];
        N = k.normal[v];
    }
    const bool src = is_source(N);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(src);
    if (b == 0ull) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(total, (uint32_t)__popcll(b));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if (!src) return;
    const uint32_t s = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    write_source(k, s, v, v % k.n, (v / k.n) % k.n, v / (k.n * k.n), N);
}

__global__ void __launch_bounds__(256) k_bounce_count_list(const float4* __restrict__ normal,
                                                           const uint32_t* __restrict__ occ_list,
                                                           const uint32_t* __restrict__ occ_count, uint32_t* total) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool src = false;
    if (i < *occ_count) src = is_source(normal[occ_list[i]]);
    const unsigned long long b = __builtin_amdgcn_ballot_w64(src);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(total, (uint32_t)__popcll(b));
}

__global__ void __launch_bounds__(256) k_bounce_save(const uint32_t* __restrict__ vox, uint32_t n_src,
                                                     const float4* __restrict__ pyr, uint32_t n,
                                                     float4* __restrict__ l0) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s < n_src) l0[s] = pyr[l0_texel(vox[s], n)];
}

// L.rgb = L0.rgb + A.rgb * I.rgb (one multiply, one add; the unit is compiled with
// -ffp-contract=off), L.a = L0.a
__global__ void __launch_bounds__(256) k_bounce_add(const uint32_t* __restrict__ vox, uint32_t n_src,
                                                    uint32_t tiles_x, const float4* __restrict__ l0,
                                                    const float4* __restrict__ albedo_occ,
                                                    const float4* __restrict__ diff, float4* __restrict__ pyr,
                                                    uint32_t n) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n_src) return;
    const uint32_t v = vox[s];
    const float4 L = l0[s], A = albedo_occ[v], I = diff[bounce_pixel(s, tiles_x)];
    pyr[l0_texel(v, n)] = make_float4(L.x + A.x * I.x, L.y + A.y * I.y, L.z + A.z * I.z, L.w);
}

// sky light: L.rgb = L.rgb + A.rgb * Sk.rgb on level 0 itself (one multiply, one add), L.a kept
__global__ void __launch_bounds__(256) k_bounce_add_plane(const uint32_t* __restrict__ vox, uint32_t n_src,
                                                          uint32_t tiles_x, const float4* __restrict__ albedo_occ,
                                                          const float4* __restrict__ plane, float4* __restrict__ pyr,
                                                          uint32_t n) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n_src) return;
    const uint32_t v = vox[s];
    float4* const dst = pyr + l0_texel(v, n);
    const float4 L = *dst, A = albedo_occ[v], I = plane[bounce_pixel(s, tiles_x)];
    *dst = make_float4(L.x + A.x * I.x, L.y + A.y * I.y, L.z + A.z * I.z, L.w);
}

template <typename T>
hipError_t grow(vct_ctx* c, T*& p, size_t& cap, size_t count) {
    if (cap >= count) return hipSuccess;
    if (p) {
        hipError_t e = hipStreamSynchronize(c->stream);   // a queued bounce may still use it
        if (e != hipSuccess) return e;
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess) cap = count;
    return e;
}

}  // namespace

hipError_t bounce_sources(vct_ctx* c) {
    Grid& g = c->grid;
    Bounce& b = c->bounce;
    if (b.built && b.epoch == c->grid_epoch) return hipSuccess;
    b.built = false;
    hipStream_t s = c->stream;
    hipError_t e;
    if (b.profile) {
        for (hipEvent_t& ev : b.ev)
            if (!ev && (e = hipEventCreate(&ev)) != hipSuccess) return e;
        if ((e = hipEventRecord(b.ev[0], s)) != hipSuccess) return e;
    }
    SourceK k;
    k.occ_bits = g.occ_bits;
    k.normal = g.normal;
    k.n = g.n;
    k.g0x = g.g0[0]; k.g0y = g.g0[1]; k.g0z = g.g0[2];
    k.hh = g.extent / (float)g.n;
    k.tiles_x = 1;
    k.vox = nullptr; k.pos = nullptr; k.nrm = nullptr;
    const uint32_t R = g.n < 16u ? g.n : 16u, nr = g.n / R, regions = nr * nr * nr;
    const size_t nv = (size_t)g.n * g.n * g.n;
    const uint32_t list_blocks = (uint32_t)((nv + 255) / 256);   // occ_list holds at most n^3 entries
    if ((e = grow(c, b.region, b.region_cap, (size_t)regions + 2)) != hipSuccess) return e;
    uint32_t* total = b.region + regions;
    if (b.order) {
        hipLaunchKernelGGL(k_bounce_regions, dim3(regions), dim3(256), 0, s, k, R, (const uint32_t*)nullptr, b.region);
        hipLaunchKernelGGL(k_bounce_scan, dim3(1), dim3(1024), 0, s, b.region, regions);
    } else {
        if ((e = hipMemsetAsync(total, 0, 8, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_bounce_count_list, dim3(list_blocks), dim3(256), 0, s, g.normal, g.occ_list, g.occ_count,
                           total);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t n_src = 0;
    if ((e = hipMemcpyAsync(&n_src, total, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if ((size_t)n_src > nv) return hipErrorUnknown;
    // the frame K4 traces: whole 64x64 tiles in one column (a frame is at most 65536 pixels
    // high: 4 M sources), else in the fewest columns that keep it so
    const uint32_t tiles = (n_src + VCT_TILE * VCT_TILE - 1u) / (VCT_TILE * VCT_TILE);
    b.tiles_x = (tiles + 1023u) / 1024u;
    if (b.tiles_x == 0) b.tiles_x = 1;
    b.tiles_y = (tiles + b.tiles_x - 1u) / b.tiles_x;
    if (b.tiles_y == 0) b.tiles_y = 1;
    b.n_src = n_src;
    const size_t px = (size_t)b.tiles_x * b.tiles_y * VCT_TILE * VCT_TILE;
    if (n_src) {
        size_t cap4 = b.px_cap * 4;
        if ((e = grow(c, b.vox, b.src_cap, n_src)) != hipSuccess) return e;
        if ((e = grow(c, b.l0, b.l0_cap, n_src)) != hipSuccess) return e;
        if ((e = grow(c, b.gbuf, cap4, px * 4)) != hipSuccess) return e;
        b.px_cap = cap4 / 4;
        k.tiles_x = b.tiles_x;
        k.vox = b.vox;
        k.pos = b.gbuf;
        k.nrm = b.gbuf + b.px_cap;
        // every pixel a background record (P.w = 0), then the sources over the first n_src
        if ((e = hipMemsetAsync(k.pos, 0, px * sizeof(float4), s)) != hipSuccess) return e;
        if (b.order) {
            hipLaunchKernelGGL(k_bounce_regions, dim3(regions), dim3(256), 0, s, k, R, (const uint32_t*)b.region,
                               (uint32_t*)nullptr);
        } else {
            hipLaunchKernelGGL(k_bounce_list, dim3(list_blocks), dim3(256), 0, s, k, (const uint32_t*)g.occ_list,
                               (const uint32_t*)g.occ_count, total + 1);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (b.profile) {
        if ((e = hipEventRecord(b.ev[1], s)) != hipSuccess) return e;
        if ((e = hipEventSynchronize(b.ev[1])) != hipSuccess) return e;
        if ((e = hipEventElapsedTime(&b.ms[0], b.ev[0], b.ev[1])) != hipSuccess) return e;
    }
    b.epoch = c->grid_epoch;
    b.built = true;
    return hipSuccess;
}

hipError_t launch_bounce_save(vct_ctx* c) {
    const Bounce& b = c->bounce;
    if (!b.n_src) return hipSuccess;
    hipLaunchKernelGGL(k_bounce_save, dim3((b.n_src + 255u) / 256u), dim3(256), 0, c->stream, (const uint32_t*)b.vox,
                       b.n_src, (const float4*)c->grid.pyr, c->grid.n, b.l0);
    return hipGetLastError();
}

hipError_t launch_bounce_gather(vct_ctx* c) {
    const Bounce& b = c->bounce;
    if (!b.n_src) return hipSuccess;
    vct_trace_args a{};
    a.pos4 = (const float*)b.gbuf;
    a.nrm4 = (const float*)(b.gbuf + b.px_cap);
    a.alb4 = a.nrm4;                             // roughness belongs to the specular cone: never read
    a.diffuse4 = (float*)(b.gbuf + 2 * b.px_cap);
    a.spec4 = (float*)(b.gbuf + 3 * b.px_cap);
    a.width = b.tiles_x * VCT_TILE;
    a.height = b.tiles_y * VCT_TILE;
    return launch_trace(c, &a, b.form);
}

hipError_t launch_bounce_accumulate(vct_ctx* c) {
    const Bounce& b = c->bounce;
    if (!b.n_src) return hipSuccess;
    hipLaunchKernelGGL(k_bounce_add, dim3((b.n_src + 255u) / 256u), dim3(256), 0, c->stream, (const uint32_t*)b.vox,
                       b.n_src, b.tiles_x, (const float4*)b.l0, (const float4*)c->grid.albedo_occ,
                       (const float4*)(b.gbuf + 2 * b.px_cap), c->grid.pyr, c->grid.n);
    return hipGetLastError();
}

hipError_t launch_bounce_add_plane(vct_ctx* c, int plane) {
    const Bounce& b = c->bounce;
    if (!b.n_src) return hipSuccess;
    hipLaunchKernelGGL(k_bounce_add_plane, dim3((b.n_src + 255u) / 256u), dim3(256), 0, c->stream,
                       (const uint32_t*)b.vox, b.n_src, b.tiles_x, (const float4*)c->grid.albedo_occ,
                       (const float4*)(b.gbuf + (size_t)plane * b.px_cap), c->grid.pyr, c->grid.n);
    return hipGetLastError();
}

void bounce_free(vct_ctx* c) {
    Bounce& b = c->bounce;
    if (b.vox) (void)hipFree(b.vox);
    if (b.l0) (void)hipFree(b.l0);
    if (b.gbuf) (void)hipFree(b.gbuf);
    if (b.region) (void)hipFree(b.region);
    for (hipEvent_t ev : b.ev)
        if (ev) (void)hipEventDestroy(ev);
    b = Bounce{};
}

}  // namespace vct

// Tool hook (not part of the public headers; tools/bounce_bench.py): form / order >= 0 set
// the compiled K4 form of the gather (0 union, 1 occupancy) and the source order (1 region
// runs, 0 occ_list order; the list is rebuilt); profile != 0 times the stages of the
// following calls with events (the call then waits for its last stage).  ms4 (nullable)
// receives the last list build and the last bounce's gather, accumulate and K3 times.
extern "C" int vct_debug_bounce(vct_ctx* c, int form, int order, int profile, float* ms4) {
    if (!c) return -1;
    if (form >= 0) c->bounce.form = form & 1;
    if (order >= 0) {
        c->bounce.order = order & 1;
        c->bounce.built = false;
    }
    c->bounce.profile = profile != 0;
    if (ms4)
        for (int i = 0; i < 4; ++i) ms4[i] = c->bounce.ms[i];
    return 0;
}
