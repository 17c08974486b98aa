// vct_objects.hip — the object set (include/vct_objects.h; include/vct_spec.h "dynamic
// objects"): rigid meshes registered once in object space, each placed by a matrix, of which an
// update retracts and voxelizes again the ones it names and no other.
//
// The context keeps, per triangle of the set, K1's setup record for the pose in place (TriGeom,
// the six 16.16 values, the candidate count).  What a triangle added can be subtracted again
// exactly (vct_dynamic.hip), so an update of M triangles builds a compact list of 2 M records
// -- slot j < M: triangle j's record as it stands, to be retracted; slot M + j: its record under
// the new pose, to be added -- and walks it once:
//   k_obj_setup       one lane per moved triangle: finds its object in the update's table (a
//                     search over the named objects' triangle prefix), copies the old record to
//                     slot j, transforms the three vertices by the transform rule, runs
//                     k_dyn_setup's arithmetic on them (vct_voxel_sat.h) and writes the new record
//                     to the persistent array and to slot M + j, and the triangle the G-buffer
//                     passes read to its fixed index of Mesh::tri.  A hidden object writes rejected
//                     records and zero triangles.  The first lanes also keep the per-object
//                     visibility words.
//   k_dyn_scan        the exclusive scan of the 2 M counts (K1's three kernels above kSmallScan).
//   k_obj_candidates  one lane per 2 candidates of the flat list, as k_dyn_candidates: K1's walk,
//                     then the hit's values, negated for a slot below M, into the record in the
//                     layout the grid has (4 or 7 atomics, none returning), and the voxel's bit in
//                     the scratch mask.  The adds are modular and commute: both signs are in
//                     flight in one launch.
//   k_obj_list        the mask's bits as the fix-up list; the mask is cleared word by word on
//                     the way (it is all zero between updates).
//   k_dyn_fixup, k_dyn_occ_list, K3's live blocks: the layer's (vct_dynamic_sat.h).
//   k_obj_scatter_poses (vct_motion.hip): the update's poses into the set's per-object array,
//                     which include/vct_motion.h reads; queued before the wait.
// One wait for the stream, at the end: the redo flag, the stats and K3's live-block count.
// Redo, when only a subset moved: retract what this update added (the slots from M on, packed),
// k_dyn_unpack the occupied records, add those slots again in the seven-atomic form, fix the
// listed voxels up again.  Nothing in an update is proportional to the set's triangle count or
// to n^3 x record size: the grid-sized passes are over bit words.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "vct_internal.h"
#include "vct_dynamic_sat.h"

namespace vct {
namespace {

constexpr int kSlotTmp = 1, kSlotList = 4;   // vct_ctx::scratch, as the layer uses them
constexpr uint32_t kObjBlocks = 1024;        // blocks of the candidate pass (its total is not known on the host)
constexpr int kObjCandPerThread = 2;         // as kDynCandPerThread (vct_dynamic.hip): the pass is latency-bound
enum { kWalkBoth = 0, kWalkRetractAdded = 1, kWalkAddAgain = 2 };

struct ObjPose {      // vct_object_pose as the kernel reads it
    float m[16];
    uint32_t visible, reserved[3];
};
static_assert(sizeof(ObjPose) == 80 && sizeof(vct_object_pose) == 80, "vct_object_pose is 80 bytes");

// persistent records of n_tri triangles: geom | fix | counts | head
TriGeom* rec_geom(const Objects& o) { return (TriGeom*)o.rec; }
DynFix* rec_fix(const Objects& o) { return (DynFix*)((char*)o.rec + sizeof(TriGeom) * (size_t)o.n_tri); }
unsigned long long* rec_cnt(const Objects& o) {
    return (unsigned long long*)((char*)o.rec + (sizeof(TriGeom) + sizeof(DynFix)) * (size_t)o.n_tri);
}
DynHead* rec_head(const Objects& o) {
    return (DynHead*)((char*)o.rec + (sizeof(TriGeom) + sizeof(DynFix) + 8) * (size_t)o.n_tri);
}
// an update's table of n named objects: prefix[n + 1] | tri0[n] | id[n] | (16-byte aligned) poses[n]
size_t tab_pose_offset(uint32_t n) { return (((size_t)3 * n + 1) * 4 + 15) & ~(size_t)15; }
size_t tab_bytes(uint32_t n) { return tab_pose_offset(n) + (size_t)n * sizeof(ObjPose); }

// the transform rule (vct_spec.h "dynamic objects"): one rounding per operation, no fma
__device__ __forceinline__ float xform_row(float a, float b, float c, float d, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)), __fmul_rn(c, z)), d);
}

__global__ void __launch_bounds__(256) k_obj_setup(const float* __restrict__ pos, const uint32_t* __restrict__ idx,
                                                   const uint32_t* __restrict__ mat, const float4* __restrict__ kd,
                                                   const uint32_t* __restrict__ prefix, const uint32_t* __restrict__ tri0,
                                                   const uint32_t* __restrict__ ids, const ObjPose* __restrict__ poses,
                                                   uint32_t n_named, uint32_t n_moved, int n, float g0x, float g0y,
                                                   float g0z, float inv_h, TriGeom* __restrict__ pgeom,
                                                   DynFix* __restrict__ pfix, unsigned long long* __restrict__ pcnt,
                                                   TriGeom* __restrict__ cgeom, DynFix* __restrict__ cfix,
                                                   unsigned long long* __restrict__ ccnt, float4* __restrict__ mesh_tri,
                                                   uint32_t* __restrict__ vis, DynHead* __restrict__ head) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_named) {   // the object's visibility word, and the change of the visible count
        const uint32_t now = poses[j].visible != 0u ? 1u : 0u, was = vis[ids[j]];
        vis[ids[j]] = now;
        if (now != was) atomicAdd(&head->pad, now - was);
    }
    if (j >= n_moved) return;
    // the named object holding moved triangle j: the last k with prefix[k] <= j
    uint32_t lo = 0, hi = n_named;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (prefix[mid] <= j) lo = mid; else hi = mid;
    }
    const uint32_t t = tri0[lo] + (j - prefix[lo]);   // the triangle's index in the set
    const ObjPose& ps = poses[lo];
    // the record in place: this update's retraction
    cgeom[j] = pgeom[t];
    cfix[j] = pfix[t];
    ccnt[j] = pcnt[t];
    const uint32_t a = n_moved + j;
    const float4 alb = kd ? kd[mat[t]] : make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    const float z[3] = {0.0f, 0.0f, 0.0f};
    float p[3][3], q[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* src = pos + 3 * (size_t)idx[3 * (size_t)t + k];
        const float x = src[0], y = src[1], w = src[2];
        p[k][0] = xform_row(ps.m[0], ps.m[4], ps.m[8], ps.m[12], x, y, w);
        p[k][1] = xform_row(ps.m[1], ps.m[5], ps.m[9], ps.m[13], x, y, w);
        p[k][2] = xform_row(ps.m[2], ps.m[6], ps.m[10], ps.m[14], x, y, w);
        q[k][0] = (p[k][0] - g0x) * inv_h;   // load_tri's q
        q[k][1] = (p[k][1] - g0y) * inv_h;
        q[k][2] = (p[k][2] - g0z) * inv_h;
    }
    if (ps.visible == 0u || !tri_finite(q)) {   // hidden, or skipped by the K1 input rule: a zero triangle
        reject_tri(pgeom, pcnt, t);
        reject_tri(cgeom, ccnt, a);
        store_mesh_tri(mesh_tri, t, z, z, z, alb, -1);
        return;
    }
    TriGeom g;
    DynFix f;
    float e1[3], e2[3];
    face_fix(p, alb, f.fix, e1, e2);
    fix_maxabs(f.fix, &head->maxabs);
    const unsigned long long cnt = tri_range(q, n, g);
    pcnt[t] = cnt;
    pgeom[t] = g;
    pfix[t] = f;
    ccnt[a] = cnt;
    cgeom[a] = g;
    cfix[a] = f;
    store_mesh_tri(mesh_tri, t, p[0], e1, e2, alb, -1);
}

// One lane = kObjCandPerThread consecutive candidates per sweep of the flat list of n_slots =
// 2 n_moved records.  A hit of a slot below n_moved is subtracted (two's complement: the modular
// inverse of what it once added), one from n_moved on is added.  mode kWalkRetractAdded /
// kWalkAddAgain (the redo path): only the slots from n_moved on, subtracted / added.
template <bool PACKED>
__global__ void __launch_bounds__(256) k_obj_candidates(const TriGeom* __restrict__ geom, const DynFix* __restrict__ fixr,
                                                        const unsigned long long* __restrict__ offs, uint32_t n_slots,
                                                        uint32_t n_moved, const DynHead* __restrict__ head, int n,
                                                        long long* __restrict__ accum,
                                                        unsigned long long* __restrict__ mask, int mode) {
    const unsigned long long total = head->total;
    const unsigned long long sweep = (unsigned long long)gridDim.x * blockDim.x * kObjCandPerThread;
    for (unsigned long long c0 = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) * kObjCandPerThread; c0 < total;
         c0 += sweep) {
        const uint32_t t0 = find_tri(offs, 0, n_slots, c0);
        for_each_hit<kObjCandPerThread>(geom, offs, n_slots, total, c0, t0,
                                        [&](uint32_t t, int vx, int vy, int vz, const float*) __attribute__((always_inline)) {
            if (mode != kWalkBoth && t < n_moved) return;
            const bool neg = mode == kWalkBoth ? t < n_moved : mode == kWalkRetractAdded;
            const size_t v = (size_t)vx + (size_t)n * ((size_t)vy + (size_t)n * (size_t)vz);
            unsigned long long* a = (unsigned long long*)(accum + 8 * v);
            const DynFix& f = fixr[t];
            if constexpr (PACKED) {
                const unsigned long long w0 = (unsigned long long)f.fix[0] + ((unsigned long long)f.fix[1] << 32);
                const unsigned long long w1 = (unsigned long long)f.fix[2] + ((unsigned long long)f.fix[3] << 32);
                const unsigned long long w2 = (unsigned long long)f.fix[4] + ((unsigned long long)f.fix[5] << 32);
                atomicAdd(a + 0, neg ? 0ull - w0 : w0);
                atomicAdd(a + 1, neg ? 0ull - w1 : w1);
                atomicAdd(a + 2, neg ? 0ull - w2 : w2);
                atomicAdd(a + 3, neg ? ~0ull : 1ull);
            } else {
#pragma unroll
                for (int i = 0; i < 6; ++i)
                    atomicAdd(a + i, neg ? 0ull - (unsigned long long)f.fix[i] : (unsigned long long)f.fix[i]);
                atomicAdd(a + 6, neg ? ~0ull : 1ull);
            }
            if (mask) atomicOr(mask + (v >> 6), 1ull << (v & 63));
        });
    }
}

// the fix-up list: the voxels the update hit, in bitmask order; the mask is left all zero
__global__ void __launch_bounds__(256) k_obj_list(unsigned long long* __restrict__ mask, size_t nwords,
                                                  uint32_t* __restrict__ list, DynHead* __restrict__ head,
                                                  uint32_t* __restrict__ occ_count) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w == 0) *occ_count = 0;   // for k_dyn_occ_list, two launches on
    const unsigned long long m = w < nwords ? mask[w] : 0ull;
    if (m) mask[w] = 0ull;
    list_block_words(m, w, list, &head->n_touched);
}

void launch_candidates(vct_ctx* c, const TriGeom* geom, const DynFix* fix, const unsigned long long* offs, uint32_t n_moved,
                       bool packed, unsigned long long* mask, int mode) {
    Grid& g = c->grid;
    if (packed)
        hipLaunchKernelGGL(k_obj_candidates<true>, dim3(kObjBlocks), dim3(256), 0, c->stream, geom, fix, offs, 2 * n_moved,
                           n_moved, rec_head(c->obj), (int)g.n, g.accum, mask, mode);
    else
        hipLaunchKernelGGL(k_obj_candidates<false>, dim3(kObjBlocks), dim3(256), 0, c->stream, geom, fix, offs, 2 * n_moved,
                           n_moved, rec_head(c->obj), (int)g.n, g.accum, mask, mode);
}

void launch_fixup(vct_ctx* c, const uint32_t* list, bool packed) {
    Grid& g = c->grid;
    const size_t nv = (size_t)g.n * g.n * g.n;
    const uint32_t lb = (uint32_t)std::min<size_t>((nv + 255) / 256, 1024);
    DynHead* head = rec_head(c->obj);
    // max|value|: the static pass's and the running maximum of everything the set ever added
    if (packed)
        hipLaunchKernelGGL(k_dyn_fixup<true>, dim3(lb), dim3(256), 0, c->stream, list, head, g.accum, g.occ_bits, g.albedo_occ,
                           g.normal, g.pyr, g.n, std::max(g.k1_maxabs, c->obj.maxabs), &head->redo);
    else
        hipLaunchKernelGGL(k_dyn_fixup<false>, dim3(lb), dim3(256), 0, c->stream, list, head, g.accum, g.occ_bits, g.albedo_occ,
                           g.normal, g.pyr, g.n, 0u, &head->redo);
}

// Places the objects ids[0 .. n) (validated: distinct, < n_objects) by d_poses (device; the
// table's own copy in the host form).  Everything before the first launch leaves the context as
// it was.
vct_status objects_move(vct_ctx* c, const uint32_t* ids, uint32_t n, const ObjPose* d_poses) {
    Grid& g = c->grid;
    Objects& o = c->obj;
    Mesh& m = c->mesh;
    hipStream_t s = c->stream;
    const size_t nv = (size_t)g.n * g.n * g.n, nwords = nv / 64;
    hipError_t e;

    // the table: the named objects' triangle prefix, first triangle and id
    uint32_t* tab = (uint32_t*)o.h_tab;
    uint32_t n_moved = 0;
    for (uint32_t j = 0; j < n; ++j) {
        tab[j] = n_moved;
        tab[n + 1 + j] = o.first[ids[j]];
        tab[2 * n + 1 + j] = ids[j];
        n_moved += o.first[ids[j] + 1] - o.first[ids[j]];
    }
    tab[n] = n_moved;
    const uint32_t n_slots = 2 * n_moved;   // n_moved <= n_tri, and 2 n_tri fits (objects_define)
    const uint32_t n_tiles = (n_slots + kScanTile - 1) / kScanTile;
    const size_t off_fix = sizeof(TriGeom) * (size_t)n_slots, off_cnt = off_fix + sizeof(DynFix) * (size_t)n_slots;
    const size_t off_offs = off_cnt + 8 * (size_t)n_slots, off_tiles = off_offs + 8 * (size_t)n_slots;
    void* tp = nullptr;
    if ((e = scratch_get(c, kSlotTmp, off_tiles + 8 * (size_t)(n_tiles + 1) + 64, &tp)) != hipSuccess) return lhip(c, e, "scratch");
    TriGeom* cgeom = (TriGeom*)tp;
    DynFix* cfix = (DynFix*)((char*)tp + off_fix);
    unsigned long long* ccnt = (unsigned long long*)((char*)tp + off_cnt);
    unsigned long long* coffs = (unsigned long long*)((char*)tp + off_offs);
    unsigned long long* tiles = (unsigned long long*)((char*)tp + off_tiles);
    void* lp = nullptr;
    if ((e = scratch_get(c, kSlotList, 256 + nv * 4, &lp)) != hipSuccess) return lhip(c, e, "scratch");
    uint32_t* list = (uint32_t*)((char*)lp + 256);

    // what vct_voxelize_dynamic invalidates; only the success path sets `voxelized` again
    g.voxelized = g.injected = g.mipped = g.bounced = g.emitted = g.skied = false;
    g.k2_coarse_ok = g.k3_sparse_ok = g.zm_valid = false;
    g.k3_live_bz = 0;
    const bool shaded = shading_live(c);   // both describe the static triangles, which stay
    const bool cutout = cutout_live(c);
    ++c->grid_epoch;
    if (shaded) c->shade.epoch = c->grid_epoch;
    if (cutout) c->cut.epoch = c->grid_epoch;
    o.live = false;

    DynHead* head = rec_head(o);
    const size_t tab_words = ((size_t)3 * n + 1) * 4;
    if ((e = hipMemcpyAsync(o.tab, o.h_tab, d_poses ? tab_words : tab_bytes(n), hipMemcpyHostToDevice, s)) != hipSuccess)
        return lhip(c, e, "upload table");
    if ((e = hipMemsetAsync(head, 0, sizeof(DynHead), s)) != hipSuccess) return lhip(c, e, "memset");
    const uint32_t* d_tab = (const uint32_t*)o.tab;
    const ObjPose* poses = d_poses ? d_poses : (const ObjPose*)((const char*)o.tab + tab_pose_offset(n));
    const bool packed = g.accum_packed;
    hipLaunchKernelGGL(k_obj_setup, dim3((std::max(n_moved, n) + 255) / 256), dim3(256), 0, s, o.pos, o.idx, o.mat, o.kd, d_tab,
                       d_tab + n + 1, d_tab + 2 * n + 1, poses, n, n_moved, (int)g.n, g.g0[0], g.g0[1], g.g0[2], g.inv_h,
                       rec_geom(o), rec_fix(o), rec_cnt(o), cgeom, cfix, ccnt, m.tri + 4 * (size_t)o.n_static, o.vis, head);
    if (n_moved) {
        if (n_slots <= kSmallScan) {
            hipLaunchKernelGGL(k_dyn_scan, dim3(1), dim3(kScanBlock), 0, s, ccnt, coffs, n_slots, &head->total);
        } else {
            launch_count_scan(s, ccnt, coffs, tiles, n_slots, &head->total);
        }
        launch_candidates(c, cgeom, cfix, coffs, n_moved, packed, o.mask, kWalkBoth);
    }
    const uint32_t wb = (uint32_t)((nwords + 255) / 256);
    hipLaunchKernelGGL(k_obj_list, dim3(wb), dim3(256), 0, s, o.mask, nwords, list, head, g.occ_count);
    launch_fixup(c, list, packed);
    hipLaunchKernelGGL(k_dyn_occ_list, dim3(wb), dim3(256), 0, s, g.occ_bits, nwords, g.occ_list, g.occ_count);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "objects_update");
    if ((e = launch_k3_live(c)) != hipSuccess) return lhip(c, e, "K3 live blocks");
    // the set remembers the poses (vct_motion.h); queued before the wait, which is what lets the
    // caller of the device form reuse its poses once the call has returned.  An update that fails
    // after this point has written the array already; it leaves `live` false, so nothing reads it
    objects_scatter_poses(s, d_tab + 2 * n + 1, poses, n, o.poses);
    if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "objects_update: poses");
    if ((e = hipMemcpyAsync(o.h_head, head, sizeof(DynHead), hipMemcpyDeviceToHost, s)) != hipSuccess) return lhip(c, e, "read back");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return lhip(c, e, "objects_update sync");
    const DynHead h = *(const DynHead*)o.h_head;
    if ((size_t)h.n_touched > nv) return lfail(c, VCT_EDEVICE, "objects_update: count out of range");
    o.maxabs = std::max(o.maxabs, h.maxabs);
    if (packed && (h.redo & kK1ErrRedo)) {
        // the packed records cannot hold the union: take out again what this update added (exact,
        // whatever overflowed meanwhile), unpack what is left, and add it in the seven-atomic form
        if (h.total) launch_candidates(c, cgeom, cfix, coffs, n_moved, true, nullptr, kWalkRetractAdded);
        const uint32_t lb = (uint32_t)std::min<size_t>((nv + 255) / 256, 4096);
        hipLaunchKernelGGL(k_dyn_unpack, dim3(lb), dim3(256), 0, s, g.occ_list, g.occ_count, g.accum);
        g.accum_packed = false;
        if (h.total) launch_candidates(c, cgeom, cfix, coffs, n_moved, false, nullptr, kWalkAddAgain);
        launch_fixup(c, list, false);
        if ((e = hipGetLastError()) != hipSuccess) return lhip(c, e, "objects_update (unpacked)");
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return lhip(c, e, "objects_update sync");
    }
    o.n_visible += h.pad;   // two's complement: gained minus lost
    o.last_moved = n_moved;
    o.last_cand = h.total;
    o.last_touched = h.n_touched;
    o.live = true;
    o.epoch = c->grid_epoch;
    g.voxelized = true;
    return VCT_OK;
}

void release(Objects& o) {
    for (void* p : {(void*)o.pos, (void*)o.idx, (void*)o.mat, (void*)o.kd, o.rec, (void*)o.vis, (void*)o.mask, o.tab, o.poses,
                    (void*)o.d_first})
        if (p) (void)hipFree(p);
    if (o.h_tab) (void)hipHostFree(o.h_tab);
    if (o.h_head) (void)hipHostFree(o.h_head);
    o = Objects{};
}

// what both update forms check: state, the ids
vct_status update_args(vct_ctx* c, const uint32_t* ids, const void* poses, uint32_t n) {
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "objects_update without a static grid (voxelize first)");
    if (!objects_live(c)) return lfail(c, VCT_ESTATE, "objects_update without an object set (vct_objects_define first)");
    if (n == 0) return VCT_OK;
    if (!ids || !poses) return lfail(c, VCT_EINVAL, "objects_update: null ids or poses");
    if (n > c->obj.n_objects) return lfail(c, VCT_EINVAL, "objects_update: more ids than objects (an id is named twice)");
    std::vector<uint8_t> seen(c->obj.n_objects, 0);
    for (uint32_t j = 0; j < n; ++j) {
        if (ids[j] >= c->obj.n_objects)
            return lfail(c, VCT_EINVAL, "objects_update: id " + std::to_string(ids[j]) + " >= n_objects");
        if (seen[ids[j]]) return lfail(c, VCT_EINVAL, "objects_update: id " + std::to_string(ids[j]) + " named twice");
        seen[ids[j]] = 1;
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    return VCT_OK;
}

}  // namespace

void objects_free(vct_ctx* c) { release(c->obj); }

}  // namespace vct

using namespace vct;

extern "C" vct_status vct_objects_define(vct_ctx* c, const vct_object_mesh* meshes, uint32_t n_objects, const float* kd4,
                                         uint32_t n_mat) {
    if (!c) return VCT_EINVAL;
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "objects_define without a static grid (voxelize first)");
    if (layer_in_place(c))
        return lfail(c, VCT_ESTATE, "objects_define with a dynamic layer in place (vct_voxelize_dynamic with no triangles removes it)");
    if (n_objects > VCT_MAX_OBJECTS) return lfail(c, VCT_EINVAL, "objects_define: n_objects > VCT_MAX_OBJECTS");
    if (n_objects && !meshes) return lfail(c, VCT_EINVAL, "objects_define: null meshes");
    if (kd4 && n_mat == 0) return lfail(c, VCT_EINVAL, "objects_define: material_kd4 with n_materials == 0");
    const uint32_t n_static = static_triangles(c);
    uint64_t n_tri = 0, n_verts = 0;
    for (uint32_t k = 0; k < n_objects; ++k) {
        const vct_object_mesh& ms = meshes[k];
        const std::string who = "objects_define: object " + std::to_string(k) + ": ";
        if (ms.vertex_stride < 12 || ms.vertex_stride % 4 != 0)
            return lfail(c, VCT_EINVAL, who + "vertex_stride < 12 or not a multiple of 4");
        if (ms.n_idx % 3 != 0) return lfail(c, VCT_EINVAL, who + "n_idx must be a multiple of 3");
        if ((ms.n_idx && !ms.idx) || (ms.n_verts && !ms.verts)) return lfail(c, VCT_EINVAL, who + "null vertex or index array");
        for (uint32_t i = 0; i < ms.n_idx; ++i)
            if (ms.idx[i] >= ms.n_verts) return lfail(c, VCT_EINVAL, who + "vertex index out of range");
        for (uint32_t t = 0; t < ms.n_idx / 3; ++t) {
            const uint32_t m = ms.tri_material ? ms.tri_material[t] : 0u;
            if (!kd4) continue;
            if (m >= n_mat) return lfail(c, VCT_EINVAL, who + "material index out of range");
            if (!kd_legal(kd4[4 * (size_t)m], kd4[4 * (size_t)m + 1], kd4[4 * (size_t)m + 2])) return lfail(c, VCT_EINVAL, kKdMessage);
        }
        n_tri += ms.n_idx / 3;
        n_verts += ms.n_verts;
    }
    // (twice the set's triangles are an update's compact list at most)
    if ((uint64_t)n_static + n_tri > 0xffffffffull || 2 * n_tri > 0xffffffffull || n_verts > 0xffffffffull)
        return lfail(c, VCT_EINVAL, "objects_define: too many triangles");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");

    Objects& o = c->obj;
    Mesh& m = c->mesh;
    hipStream_t s = c->stream;
    if (objects_live(c)) {   // retract the set in place: hide every visible object
        if (o.n_visible) {
            // (visibility lives on the device; hiding a hidden object retracts rejected records: nothing)
            std::vector<uint32_t> ids(o.n_objects);
            for (uint32_t k = 0; k < o.n_objects; ++k) ids[k] = k;
            ObjPose* hp = (ObjPose*)((char*)o.h_tab + tab_pose_offset(o.n_objects));
            std::memset(hp, 0, sizeof(ObjPose) * (size_t)o.n_objects);
            const vct_status st = objects_move(c, ids.data(), o.n_objects, nullptr);
            if (st != VCT_OK) return st;
        }
        m.n_tri = o.n_static;
    }
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return lhip(c, e, "objects_define sync");
    release(o);
    if (n_objects == 0) return VCT_OK;

    // the meshes, packed on the host: positions, indices into them, material ids
    std::vector<float> pos(3 * (size_t)std::max<uint64_t>(n_verts, 1));
    std::vector<uint32_t> idx(3 * (size_t)std::max<uint64_t>(n_tri, 1)), mat((size_t)std::max<uint64_t>(n_tri, 1), 0u);
    o.first.assign(n_objects + 1, 0u);
    size_t v0 = 0, t0 = 0;
    for (uint32_t k = 0; k < n_objects; ++k) {
        const vct_object_mesh& ms = meshes[k];
        for (uint32_t v = 0; v < ms.n_verts; ++v)
            std::memcpy(&pos[3 * (v0 + v)], (const char*)ms.verts + (size_t)v * ms.vertex_stride, 12);
        for (uint32_t i = 0; i < ms.n_idx; ++i) idx[3 * t0 + i] = (uint32_t)(v0 + ms.idx[i]);
        for (uint32_t t = 0; t < ms.n_idx / 3; ++t) mat[t0 + t] = ms.tri_material ? ms.tri_material[t] : 0u;
        o.first[k] = (uint32_t)t0;
        v0 += ms.n_verts;
        t0 += ms.n_idx / 3;
    }
    o.first[n_objects] = (uint32_t)t0;
    o.n_objects = n_objects;
    o.n_tri = (uint32_t)n_tri;
    o.n_mat = n_mat;
    const size_t nwords = (size_t)c->grid.n * c->grid.n * c->grid.n / 64;
    const size_t rec_bytes = (sizeof(TriGeom) + sizeof(DynFix) + 8) * (size_t)o.n_tri + sizeof(DynHead);
    const struct { void** p; size_t bytes; const void* src; } dev[] = {
        {(void**)&o.pos, pos.size() * 4, pos.data()},  {(void**)&o.idx, idx.size() * 4, idx.data()},
        {(void**)&o.mat, mat.size() * 4, mat.data()},  {(void**)&o.kd, kd4 ? (size_t)n_mat * 16 : 0, kd4},
        {&o.rec, rec_bytes, nullptr},                  {(void**)&o.vis, (size_t)n_objects * 4, nullptr},
        {(void**)&o.mask, nwords * 8, nullptr},        {&o.tab, tab_bytes(n_objects), nullptr},
        {&o.poses, sizeof(ObjPose) * (size_t)n_objects, nullptr},
        {(void**)&o.d_first, ((size_t)n_objects + 1) * 4, o.first.data()}};
    vct_status st = VCT_OK;
    for (const auto& d : dev) {
        if (!d.bytes) continue;
        if ((e = hipMalloc(d.p, d.bytes)) != hipSuccess) { st = lhip(c, e, "hipMalloc object set"); break; }
        e = d.src ? hipMemcpyAsync(*d.p, d.src, d.bytes, hipMemcpyHostToDevice, s) : hipMemsetAsync(*d.p, 0, d.bytes, s);
        if (e != hipSuccess) { st = lhip(c, e, "upload object set"); break; }
    }
    if (st == VCT_OK && (e = hipHostMalloc(&o.h_tab, tab_bytes(n_objects), hipHostMallocDefault)) != hipSuccess)
        st = lhip(c, e, "hipHostMalloc");
    if (st == VCT_OK && (e = hipHostMalloc(&o.h_head, sizeof(DynHead), hipHostMallocDefault)) != hipSuccess)
        st = lhip(c, e, "hipHostMalloc");
    // the set's triangles behind the static ones: zero triangles, which no ray hits
    const size_t all_tri = std::max<size_t>((size_t)n_static + o.n_tri, 1);
    if (st == VCT_OK) st = grow_keeping(c, m.tri, m.cap, all_tri * 4 * sizeof(float4), (size_t)n_static * 4 * sizeof(float4));
    if (st == VCT_OK && m.textured)   // the entries exist (the set's triangles have no diffuse map: never read)
        st = grow_keeping(c, m.uv, m.uv_cap, all_tri * 2 * sizeof(float4), (size_t)n_static * 2 * sizeof(float4));
    if (st == VCT_OK && o.n_tri) {
        e = hipMemsetAsync(m.tri + 4 * (size_t)n_static, 0, (size_t)o.n_tri * 4 * sizeof(float4), s);
        if (e == hipSuccess && m.textured) e = hipMemsetAsync(m.uv + 2 * (size_t)n_static, 0, (size_t)o.n_tri * 2 * sizeof(float4), s);
        if (e != hipSuccess) st = lhip(c, e, "memset");
    }
    // (the host vectors are pageable: the copies have been staged; the wait covers the fills)
    if (st == VCT_OK && (e = hipStreamSynchronize(s)) != hipSuccess) st = lhip(c, e, "objects_define sync");
    if (st != VCT_OK) {
        (void)hipStreamSynchronize(s);
        release(o);
        return st;
    }
    o.n_static = n_static;
    o.live = true;
    o.epoch = c->grid_epoch;
    m.n_tri = n_static + o.n_tri;
    return VCT_OK;
}

extern "C" vct_status vct_objects_update(vct_ctx* c, const uint32_t* ids, const vct_object_pose* poses, uint32_t n) {
    if (!c) return VCT_EINVAL;
    const vct_status st = update_args(c, ids, poses, n);
    if (st != VCT_OK || n == 0) return st;
    for (uint32_t j = 0; j < n; ++j)
        if (poses[j].visible > 1 || poses[j].reserved[0] || poses[j].reserved[1] || poses[j].reserved[2])
            return lfail(c, VCT_EINVAL, "objects_update: pose " + std::to_string(j) + ": visible > 1 or reserved != 0");
    std::memcpy((char*)c->obj.h_tab + tab_pose_offset(n), poses, sizeof(ObjPose) * (size_t)n);
    return objects_move(c, ids, n, nullptr);
}

extern "C" vct_status vct_objects_update_device(vct_ctx* c, const uint32_t* ids, const vct_object_pose* poses, uint32_t n) {
    if (!c) return VCT_EINVAL;
    const vct_status st = update_args(c, ids, poses, n);
    if (st != VCT_OK || n == 0) return st;
    if ((uintptr_t)poses & 15) return lfail(c, VCT_EINVAL, "objects_update_device: poses must be 16-byte aligned");
    return objects_move(c, ids, n, (const ObjPose*)poses);
}

extern "C" vct_status vct_objects_get_stats(vct_ctx* c, vct_objects_stats* out) {
    if (!c || !out) return c ? lfail(c, VCT_EINVAL, "objects_get_stats: null output") : VCT_EINVAL;
    if (!c->grid.voxelized) return lfail(c, VCT_ESTATE, "objects_get_stats before voxelize");
    std::memset(out, 0, sizeof(*out));
    if (!objects_live(c)) return VCT_OK;
    const Objects& o = c->obj;
    out->n_objects = o.n_objects;
    out->n_triangles = o.n_tri;
    out->n_visible = o.n_visible;
    out->last_moved_triangles = o.last_moved;
    out->last_candidates = o.last_cand;
    out->last_touched_voxels = o.last_touched;
    return VCT_OK;
}
