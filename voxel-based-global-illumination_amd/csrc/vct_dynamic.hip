// vct_dynamic.hip — the dynamic layer (include/vct_dynamic.h; include/vct_spec.h "dynamic
// layer"): one set of triangles on top of the static grid that is replaced without
// voxelizing the scene again.
//
// K1's state is integer sums accumulated with order-independent atomics, so what a triangle
// added can be subtracted again exactly (the adds are modulo 2^64, in the packed words too,
// whatever carried between their halves meanwhile).  An update therefore costs what the old
// and the new layer cost, not what the scene costs:
//   k_dyn_setup       one lane per new triangle: k1_tri_setup's arithmetic for a Kd material,
//                     from the same pieces (vct_voxel_sat.h: q, candidate range, the six 16.16
//                     values, the triangle for the G-buffer passes behind the static ones), the
//                     error word and max|value|.  The records are kept in the context: they
//                     are the next update's retraction.
//   k_dyn_scan        the exclusive scan of the candidate counts, one block (a large layer
//                     takes K1's three scan kernels, vct_voxel_sat.h).
//   k_dyn_candidates  one lane per 2 (triangle, voxel) candidates, grid-stride over the flat
//                     list (the total stays on the device: nothing is read back before the
//                     launch): K1's walk (for_each_hit, vct_voxel_sat.h), then the hit's values
//                     times `sign` into the record in the layout the grid has (4 or 7 atomics,
//                     none returning).  The old
//                     layer's records run with sign -1, the new layer's with +1; the +1 pass
//                     also sets the voxel's bit in the layer's bit mask (no first-hit logic:
//                     with both signs in flight a count of 0 proves nothing).
//   k_dyn_list        the voxels of old mask | new mask as a list (k2_list's scheme), and the
//                     number of voxels the new layer hit.
//   k_dyn_fixup       one lane per listed voxel: count 0 -> vacate (occupancy bit, albedo,
//                     normal and level-0 texel to zero; the record is all zero already), else
//                     set the bit and resolve with resolve_voxel.  A packed record whose
//                     count x max|value| (the larger of the static pass's and the layer's)
//                     could reach 2^31 raises the redo flag instead.
//   k_dyn_occ_list    the occupied list for the new occupancy; then K3's live blocks.
// One wait for the stream, at the end: error word, redo flag, counts.  Redo (rare; the result
// is the same either way): retract the new layer again, k_dyn_unpack the occupied records in
// place into the seven-atomic layout, add it unpacked and fix the listed voxels up again.
// Nothing here is proportional to n^3 x record size or to the static triangle count: the
// grid-sized passes are over bit words (n^3 / 8 bytes each).
// k_dyn_scan, k_dyn_fixup, k_dyn_occ_list and k_dyn_unpack are in vct_dynamic_sat.h, which the
// object set (vct_objects.hip) shares.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include "vct_internal.h"
#include "vct_dynamic_sat.h"

namespace vct {
namespace {

constexpr int kSlotTmp = 1, kSlotList = 4;   // vct_ctx::scratch: K1's temps, K2's work list (same sizes)
constexpr uint32_t kAddBlocks = 1024;        // blocks of the +1 pass (its total is not known on the host)
// Candidates per lane.  K1 takes 8 (kCandPerThread) to amortise its triangle search over a
// scene's millions of candidates; a layer has tens of thousands, which at 8 per lane fill a
// few dozen waves that each walk a chain of dependent loads: the pass is latency-bound, so
// fewer candidates per lane and more waves (tools/dynamic_bench.py)
constexpr int kDynCandPerThread = 2;

constexpr size_t kRecBytes = sizeof(TriGeom) + sizeof(DynFix) + 8;   // per triangle
TriGeom* rec_geom(const DynLayer& l) { return (TriGeom*)l.rec; }
DynFix* rec_fix(const DynLayer& l) { return (DynFix*)((char*)l.rec + sizeof(TriGeom) * l.cap); }
unsigned long long* rec_offs(const DynLayer& l) {
    return (unsigned long long*)((char*)l.rec + (sizeof(TriGeom) + sizeof(DynFix)) * l.cap);
}
DynHead* rec_head(const DynLayer& l) { return (DynHead*)((char*)l.rec + kRecBytes * l.cap); }

// k1_tri_setup (vct_voxelize.hip) for a Kd material: the same pieces, without the diffuse maps
__global__ void __launch_bounds__(256) k_dyn_setup(const char* __restrict__ verts, uint32_t stride, uint32_t n_verts,
                                                   const uint32_t* __restrict__ idx, uint32_t n_tri,
                                                   const uint32_t* __restrict__ mat, const float4* __restrict__ kd,
                                                   uint32_t n_mat, int n, float g0x, float g0y, float g0z, float inv_h,
                                                   TriGeom* __restrict__ geom, DynFix* __restrict__ fixo,
                                                   unsigned long long* __restrict__ counts,
                                                   float4* __restrict__ mesh_tri, DynHead* __restrict__ head) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tri) return;
    const uint32_t m = mat ? mat[t] : 0u;
    const float z[3] = {0.0f, 0.0f, 0.0f};
    uint32_t vi[3];
    float p[3][3], q[3][3];
    if ((kd && m >= n_mat) || !load_tri(verts, stride, n_verts, idx, t, g0x, g0y, g0z, inv_h, vi, p, q)) {
        atomicOr(&head->err, kK1ErrIndex);
        reject_tri(geom, counts, t);
        store_mesh_tri(mesh_tri, t, z, z, z, make_float4(0.0f, 0.0f, 0.0f, 0.0f), -1);
        return;
    }
    const float4 alb = kd ? kd[m] : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const bool kd_ok = kd_legal(alb.x, alb.y, alb.z);
    if (!kd_ok || !tri_finite(q)) {   // the K1 input rule: an error, or a skipped triangle (a zero one for the G-buffer)
        if (!kd_ok) atomicOr(&head->err, kK1ErrKd);
        reject_tri(geom, counts, t);
        store_mesh_tri(mesh_tri, t, z, z, z, alb, -1);
        return;
    }
    TriGeom g;
    DynFix f;
    float e1[3], e2[3];
    face_fix(p, alb, f.fix, e1, e2);
    fix_maxabs(f.fix, &head->maxabs);
    counts[t] = tri_range(q, n, g);
    geom[t] = g;
    fixo[t] = f;
    store_mesh_tri(mesh_tri, t, p[0], e1, e2, alb, -1);
}


// One lane = kDynCandPerThread consecutive candidates per sweep of the flat list.  NEG: the
// values are subtracted (two's complement: the modular inverse of what the +1 pass added).
// layer_bits (the +1 pass): the hit voxel's bit.
template <bool PACKED, bool NEG>
__global__ void __launch_bounds__(256) k_dyn_candidates(const TriGeom* __restrict__ geom, const DynFix* __restrict__ fixr,
                                                        const unsigned long long* __restrict__ offs, uint32_t n_tri,
                                                        const DynHead* __restrict__ head, int n,
                                                        long long* __restrict__ accum,
                                                        unsigned long long* __restrict__ layer_bits) {
    const unsigned long long total = head->total;
    const unsigned long long sweep = (unsigned long long)gridDim.x * blockDim.x * kDynCandPerThread;
    for (unsigned long long c0 = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * kDynCandPerThread; c0 < total;
         c0 += sweep) {
        // the whole list is searched: a layer is a few thousand triangles, a dozen steps
        const uint32_t t0 = find_tri(offs, 0, n_tri, c0);
        for_each_hit<kDynCandPerThread>(geom, offs, n_tri, total, c0, t0,
                                        [&](uint32_t t, int vx, int vy, int vz, const float*) __attribute__((always_inline)) {
            const size_t v = (size_t)vx + (size_t)n * ((size_t)vy + (size_t)n * (size_t)vz);
            unsigned long long* a = (unsigned long long*)(accum + 8 * v);
            const DynFix& f = fixr[t];
            if constexpr (PACKED) {
                const unsigned long long w0 = (unsigned long long)f.fix[0] + ((unsigned long long)f.fix[1] << 32);
                const unsigned long long w1 = (unsigned long long)f.fix[2] + ((unsigned long long)f.fix[3] << 32);
                const unsigned long long w2 = (unsigned long long)f.fix[4] + ((unsigned long long)f.fix[5] << 32);
                atomicAdd(a + 0, NEG ? 0ull - w0 : w0);
                atomicAdd(a + 1, NEG ? 0ull - w1 : w1);
                atomicAdd(a + 2, NEG ? 0ull - w2 : w2);
                atomicAdd(a + 3, NEG ? ~0ull : 1ull);
            } else {
#pragma unroll
                for (int i = 0; i < 6; ++i)
                    atomicAdd(a + i, NEG ? 0ull - (unsigned long long)f.fix[i] : (unsigned long long)f.fix[i]);
                atomicAdd(a + 6, NEG ? ~0ull : 1ull);
            }
            if (layer_bits) atomicOr(layer_bits + (v >> 6), 1ull << (v & 63));
        });
    }
}

// the fix-up list: the voxels of either layer, in bitmask order; and the new layer's voxel count
__global__ void __launch_bounds__(256) k_dyn_list(const unsigned long long* __restrict__ old_bits,
                                                  const unsigned long long* __restrict__ new_bits, size_t nwords,
                                                  uint32_t* __restrict__ list, DynHead* __restrict__ head,
                                                  uint32_t* __restrict__ occ_count) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w == 0) *occ_count = 0;   // for k_dyn_occ_list, two launches on (saves a 4-byte fill's launch)
    const unsigned long long nb = w < nwords ? new_bits[w] : 0ull;
    const unsigned long long ob = w < nwords ? old_bits[w] : 0ull;
    if (nb) atomicAdd(&head->n_voxels, (uint32_t)__popcll(nb));   // a layer's words are few
    list_block_words(nb | ob, w, list, &head->n_touched);
}


template <bool NEG>
void launch_candidates(vct_ctx* c, const DynLayer& l, uint32_t n_tri, uint32_t blocks, bool packed,
                       unsigned long long* layer_bits) {
    Grid& g = c->grid;
    if (packed)
        hipLaunchKernelGGL((k_dyn_candidates<true, NEG>), dim3(blocks), dim3(256), 0, c->stream, rec_geom(l), rec_fix(l),
                           rec_offs(l), n_tri, rec_head(l), (int)g.n, g.accum, layer_bits);
    else
        hipLaunchKernelGGL((k_dyn_candidates<false, NEG>), dim3(blocks), dim3(256), 0, c->stream, rec_geom(l), rec_fix(l),
                           rec_offs(l), n_tri, rec_head(l), (int)g.n, g.accum, layer_bits);
}

// blocks that cover `total` candidates in one sweep (more are swept by the kernel's loop)
uint32_t blocks_for(unsigned long long total) {
    const unsigned long long b = (total + 256ull * kDynCandPerThread - 1) / (256ull * kDynCandPerThread);
    return (uint32_t)std::min<unsigned long long>(std::max<unsigned long long>(b, 1), 1u << 20);
}

void launch_fixup(vct_ctx* c, const uint32_t* list, const DynLayer& nw, bool packed) {
    Grid& g = c->grid;
    const size_t nv = (size_t)g.n * g.n * g.n;
    const uint32_t lb = (uint32_t)std::min<size_t>((nv + 255) / 256, 1024);
    if (packed)
        hipLaunchKernelGGL(k_dyn_fixup<true>, dim3(lb), dim3(256), 0, c->stream, list, rec_head(nw), g.accum, g.occ_bits,
                           g.albedo_occ, g.normal, g.pyr, g.n, g.k1_maxabs, &rec_head(nw)->redo);
    else
        hipLaunchKernelGGL(k_dyn_fixup<false>, dim3(lb), dim3(256), 0, c->stream, list, rec_head(nw), g.accum, g.occ_bits,
                           g.albedo_occ, g.normal, g.pyr, g.n, 0u, &rec_head(nw)->redo);
}

// Replace the layer with device-resident triangles.  Everything before the first launch
// leaves the context as it was.
vct_status dynamic_update(vct_ctx* c, const void* d_verts, uint32_t stride, uint32_t n_verts, const uint32_t* d_idx,
                          uint32_t n_tri, const uint32_t* d_mat, const float4* d_kd, uint32_t n_mat) {
    Grid& g = c->grid;
    Dynamic& d = c->dyn;
    Mesh& m = c->mesh;
    hipStream_t s = c->stream;
    const size_t nv = (size_t)g.n * g.n * g.n, nwords = nv / 64;
    const bool had = dynamic_live(c);
    const uint32_t n_static = had ? d.n_static : m.n_tri;
    if ((uint64_t)n_static + n_tri > 0xffffffffull) return lfail(c, VCT_EINVAL, "voxelize_dynamic: too many triangles");
    DynLayer& old = d.layer[d.cur];
    DynLayer& nw = d.layer[1 - d.cur];
    hipError_t e;

    // memory: the two bit masks, the new layer's records, the mesh behind the static triangles
    if (!d.h_head && (e = hipHostMalloc(&d.h_head, sizeof(DynHead), hipHostMallocDefault)) != hipSuccess)
        return lhip(c, e, "hipHostMalloc");
    for (DynLayer* l : {&old, &nw})
        if (!l->bits) {
            if ((e = hipMalloc((void**)&l->bits, nwords * 8)) != hipSuccess) return lhip(c, e, "hipMalloc layer bits");
            if ((e = hipMemsetAsync(l->bits, 0, nwords * 8, s)) != hipSuccess) return lhip(c, e, "memset");
        }
    if (!nw.rec || nw.cap < n_tri) {
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return lhip(c, e, "sync");
        if (nw.rec) (void)hipFree(nw.rec);
        nw.rec = nullptr;
        nw.cap = 0;
        const size_t cap = std::max<size_t>(n_tri, 64);
        if ((e = hipMalloc(&nw.rec, kRecBytes * cap + sizeof(DynHead))) != hipSuccess)
            return lhip(c, e, "hipMalloc layer records");
        nw.cap = cap;
    }
    const size_t all_tri = std::max<size_t>((size_t)n_static + n_tri, 1);
    vct_status st = grow_keeping(c, m.tri, m.cap, all_tri * 4 * sizeof(float4), (size_t)n_static * 4 * sizeof(float4));
    if (st != VCT_OK) return st;
    if (m.textured) {   // the layer's entries exist (its triangles have no diffuse map: never read)
        st = grow_keeping(c, m.uv, m.uv_cap, all_tri * 2 * sizeof(float4), (size_t)n_static * 2 * sizeof(float4));
        if (st != VCT_OK) return st;
        if (n_tri && (e = hipMemsetAsync(m.uv + 2 * (size_t)n_static, 0, (size_t)n_tri * 2 * sizeof(float4), s)) != hipSuccess)
            return lhip(c, e, "memset uv");
    }
    const uint32_t n_tiles = (n_tri + kScanTile - 1) / kScanTile;
    void* tp = nullptr;
    if ((e = scratch_get(c, kSlotTmp, 8 * (size_t)n_tri + 8 * (size_t)(n_tiles + 1) + 64, &tp)) != hipSuccess)
        return lhip(c, e, "scratch");
    unsigned long long* cnt = (unsigned long long*)tp;
    unsigned long long* tiles = cnt + n_tri;
    void* lp = nullptr;
    if ((e = scratch_get(c, kSlotList, 256 + nv * 4, &lp)) != hipSuccess) return lhip(c, e, "scratch");
    uint32_t* list = (uint32_t*)((char*)lp + 256);

    // what voxelize_dev invalidates; only the success path sets `voxelized` again
    g.voxelized = g.injected = g.mipped = g.bounced = g.emitted = g.skied = false;
    g.k2_coarse_ok = g.k3_sparse_ok = g.zm_valid = false;
    g.k3_live_bz = 0;
    const bool shaded = shading_live(c);   // the shading set describes the static triangles, which stay
    const bool cutout = cutout_live(c);    // and so does the cutout table (the layer's triangles are opaque)
    ++c->grid_epoch;
    if (shaded) c->shade.epoch = c->grid_epoch;
    if (cutout) c->cut.epoch = c->grid_epoch;
    d.live = false;
    m.n_tri = n_static;
    if (!had) {   // no layer in place: whatever the record sets hold belongs to an earlier grid
        old.n_tri = 0;
        old.total = 0;
        if ((e = hipMemsetAsync(old.bits, 0, nwords * 8, s)) != hipSuccess) return lhip(c, e, "memset");
    }
    DynHead* head = rec_head(nw);
    if ((e = hipMemsetAsync(nw.bits, 0, nwords * 8, s)) != hipSuccess) return lhip(c, e, "memset");
    if ((e = hipMemsetAsync(head, 0, sizeof(DynHead), s)) != hipSuccess) return lhip(c, e, "memset");
    const bool packed = g.accum_packed;
    if (old.n_tri && old.total) launch_candidates<true>(c, old, old.n_tri, blocks_for(old.total), packed, nullptr);
    if (n_tri) {
        hipLaunchKernelGGL(k_dyn_setup, dim3((n_tri + 255) / 256), dim3(256), 0, s, (const char*)d_verts, stride, n_verts,
                           d_idx, n_tri, d_mat, d_kd, n_mat, (int)g.n, g.g0[0], g.g0[1], g.g0[2], g.inv_h, rec_geom(nw),
                           rec_fix(nw), cnt, m.tri + 4 * (size_t)n_static, head);
        if (n_tri <= kSmallScan) {
            hipLaunchKernelGGL(k_dyn_scan, dim3(1), dim3(kScanBlock), 0, s, cnt, rec_offs(nw), n_tri, &head->total);
        } else {
            launch_count_scan(s, cnt, rec_offs(nw), tiles, n_tri, &head->total);
        }
        launch_candidates<false>(c, nw, n_tri, kAddBlocks, packed, nw.bits);
    }
    const uint32_t wb = (uint32_t)((nwords + 255) / 256);
    hipLaunchKernelGGL(k_dyn_list, dim3(wb), dim3(256), 0, s, old.bits, nw.bits, nwords, list, head, g.occ_count);
    launch_fixup(c, list, nw, packed);
    hipLaunchKernelGGL(k_dyn_occ_list, dim3(wb), dim3(256), 0, s, g.occ_bits, nwords, g.occ_list, g.occ_count);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "voxelize_dynamic");
    if ((e = launch_k3_live(c)) != hipSuccess) return lhip(c, e, "K3 live blocks");
    // (into pinned memory: a pageable destination makes the runtime stage the 32 bytes)
    if ((e = hipMemcpyAsync(d.h_head, head, sizeof(DynHead), hipMemcpyDeviceToHost, s)) != hipSuccess) return lhip(c, e, "read back");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return lhip(c, e, "voxelize_dynamic sync");
    const DynHead h = *(const DynHead*)d.h_head;
    // a grid from out-of-range indices or an illegal Kd is partial: refused until a vct_voxelize*
    if (h.err & kK1ErrKd) return lfail(c, VCT_EINVAL, kKdMessage);
    if (h.err & kK1ErrIndex) return lfail(c, VCT_EINVAL, "voxelize_dynamic: vertex or material index out of range");
    if ((size_t)h.n_touched > nv || (size_t)h.n_voxels > nv) return lfail(c, VCT_EDEVICE, "voxelize_dynamic: count out of range");
    if (packed && (h.redo & kK1ErrRedo)) {
        // the packed records cannot hold the union: take the layer out again (exact, whatever
        // overflowed meanwhile), unpack what is left, and add the layer in the seven-atomic form
        if (n_tri && h.total) launch_candidates<true>(c, nw, n_tri, blocks_for(h.total), true, nullptr);
        const uint32_t lb = (uint32_t)std::min<size_t>((nv + 255) / 256, 4096);
        hipLaunchKernelGGL(k_dyn_unpack, dim3(lb), dim3(256), 0, s, g.occ_list, g.occ_count, g.accum);
        g.accum_packed = false;
        if (n_tri && h.total) launch_candidates<false>(c, nw, n_tri, blocks_for(h.total), false, nullptr);
        launch_fixup(c, list, nw, false);
        if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "voxelize_dynamic (unpacked)");
    }
    nw.n_tri = n_tri;
    nw.total = h.total;
    d.cur = 1 - d.cur;
    d.live = true;
    d.epoch = c->grid_epoch;
    d.n_static = n_static;
    d.n_voxels = h.n_voxels;
    m.n_tri = n_static + n_tri;
    g.voxelized = true;
    return VCT_OK;
}

vct_status dynamic_args(vct_ctx* c, const void* verts, uint32_t stride, uint32_t n_idx, const uint32_t* idx,
                        const float* kd4, uint32_t n_mat) {
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "voxelize_dynamic without a static grid (voxelize first)");
    if (objects_live(c)) return lfail(c, VCT_ESTATE, "voxelize_dynamic with an object set defined (vct_objects_define with no objects removes it)");
    if (n_idx % 3 != 0) return lfail(c, VCT_EINVAL, "voxelize_dynamic: n_idx must be a multiple of 3");
    if (n_idx > 0 && (!verts || !idx)) return lfail(c, VCT_EINVAL, "voxelize_dynamic: null vertex or index array");
    if (stride < 12 || stride % 4 != 0)
        return lfail(c, VCT_EINVAL, "voxelize_dynamic: vertex_stride < 12 or not a multiple of 4");
    if (kd4 && n_mat == 0) return lfail(c, VCT_EINVAL, "voxelize_dynamic: material_kd4 with n_materials == 0");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    return VCT_OK;
}

}  // namespace

void dynamic_free(vct_ctx* c) {
    for (DynLayer& l : c->dyn.layer) {
        if (l.rec) (void)hipFree(l.rec);
        if (l.bits) (void)hipFree(l.bits);
    }
    if (c->dyn.h_head) (void)hipHostFree(c->dyn.h_head);
    c->dyn = Dynamic{};
}

}  // namespace vct

using namespace vct;

extern "C" vct_status vct_voxelize_dynamic_device(vct_ctx* c, const void* verts, uint32_t stride, uint32_t n_verts,
                                                  const uint32_t* idx, uint32_t n_idx, const uint32_t* tri_mat,
                                                  const float* kd4, uint32_t n_mat) {
    if (!c) return VCT_EINVAL;
    vct_status st = dynamic_args(c, verts, stride, n_idx, idx, kd4, n_mat);
    if (st != VCT_OK) return st;
    if (((uintptr_t)kd4 & 15) || ((uintptr_t)verts & 3) || ((uintptr_t)idx & 3) || ((uintptr_t)tri_mat & 3))
        return lfail(c, VCT_EINVAL, "voxelize_dynamic: material_kd4 must be 16-byte, verts, idx and tri_material "
                                    "4-byte aligned");
    return dynamic_update(c, verts, stride, n_verts, idx, n_idx / 3, tri_mat, (const float4*)kd4, n_mat);
}

extern "C" vct_status vct_voxelize_dynamic(vct_ctx* c, const void* verts, uint32_t stride, uint32_t n_verts,
                                           const uint32_t* idx, uint32_t n_idx, const uint32_t* tri_mat,
                                           const float* kd4, uint32_t n_mat) {
    if (!c) return VCT_EINVAL;
    vct_status st = dynamic_args(c, verts, stride, n_idx, idx, kd4, n_mat);
    if (st != VCT_OK) return st;
    const uint32_t n_tri = n_idx / 3;
    // the Kd rule on the host, before any launch: the Kd of every material a triangle uses (an
    // out-of-range material index is the setup kernel's to report).  Unlike vct_voxelize, which
    // has nothing to fall back to, the grid and the layer in place stay as they are
    if (!used_kd_legal(tri_mat, n_tri, kd4, n_mat)) return lfail(c, VCT_EINVAL, kKdMessage);
    MeshStage ms;
    if ((st = stage_mesh(c, ms, verts, (size_t)stride * n_verts, idx, n_idx, tri_mat, kd4, "kd", nullptr, n_mat)) != VCT_OK)
        return st;
    // (dynamic_update waits for the stream after the last kernel that reads the staging buffers)
    return dynamic_update(c, ms.verts.p, stride, n_verts, (const uint32_t*)ms.idx.p, n_tri, (const uint32_t*)ms.mat.p,
                          (const float4*)ms.mats.p, n_mat);
}

// test hook (not part of the headers): 1 / 0 = the grid's records are packed / one sum per word
extern "C" int vct_debug_accum_packed(const vct_ctx* c) { return c && c->grid.accum_packed ? 1 : 0; }

extern "C" vct_status vct_dynamic_voxels(vct_ctx* c, uint32_t* n_touched) {
    if (!c || !n_touched) return c ? lfail(c, VCT_EINVAL, "dynamic_voxels: null output") : VCT_EINVAL;
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "dynamic_voxels before voxelize");
    *n_touched = dynamic_live(c) ? c->dyn.n_voxels : 0u;
    return VCT_OK;
}
