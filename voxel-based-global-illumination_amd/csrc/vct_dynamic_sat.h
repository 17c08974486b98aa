// vct_dynamic_sat.h — what the two translation units that retract and re-add K1 contributions
// share (vct_dynamic.hip: the dynamic layer; vct_objects.hip: the object set): the 16.16 values
// of a triangle and the words an update reads back, the one-block scan of a small update's
// candidate counts, the fix-up of the touched voxels, the occupied list, the in-place
// conversion of packed records, and the growth of Mesh::tri behind the static triangles.
// Like vct_voxel_sat.h, everything is internal to the including translation unit.
#pragma once
#include "vct_voxel_sat.h"

namespace vct {
namespace {

constexpr uint32_t kSmallScan = 64 * kScanTile;   // triangles up to which one block scans the counts

struct DynFix {       // 48 B
    long long fix[6]; // albedo rgb, face normal xyz in 16.16 fixed point
};

struct DynHead {      // per layer, on the device; read back once per update
    unsigned long long total;   // candidates
    uint32_t maxabs;            // largest |value| a hit adds, clamped at 2^31
    int err;                    // kK1ErrIndex | kK1ErrKd
    int redo;                   // kK1ErrRedo: a packed record may have overflowed
    uint32_t n_touched;         // entries of the fix-up list
    uint32_t n_voxels;          // voxels the layer hit
    uint32_t pad;               // the object set: visible objects gained minus lost by the update
};

// the exclusive scan of a layer's candidate counts in one block (k_scan_carry's loop over the
// counts themselves): one launch instead of three for the few thousand triangles of a layer
__global__ void __launch_bounds__(kScanBlock) k_dyn_scan(const unsigned long long* __restrict__ in,
                                                         unsigned long long* __restrict__ out, uint32_t count,
                                                         unsigned long long* __restrict__ total_out) {
    __shared__ unsigned long long sh[4];
    unsigned long long carry = 0;
    for (uint32_t b = 0; b < count; b += kScanTile) {
        const uint32_t base = b + threadIdx.x * kScanItems;
        unsigned long long v[kScanItems], s = 0, tot;
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) {
            v[i] = base + i < count ? in[base + i] : 0ull;
            s += v[i];
        }
        unsigned long long ex = carry + block_excl_scan(s, sh, tot);
#pragma unroll
        for (int i = 0; i < kScanItems; ++i) {
            if (base + i < count) out[base + i] = ex;
            ex += v[i];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

template <bool PACKED>
__global__ void __launch_bounds__(256) k_dyn_fixup(const uint32_t* __restrict__ list, const DynHead* __restrict__ head,
                                                   const long long* __restrict__ accum,
                                                   unsigned long long* __restrict__ occ_bits,
                                                   float4* __restrict__ albedo_occ, float4* __restrict__ normal,
                                                   float4* __restrict__ level0, uint32_t n, uint32_t static_maxabs,
                                                   int* __restrict__ redo) {
    const uint32_t cnt = head->n_touched;
    const uint32_t maxabs = PACKED ? max(static_maxabs, head->maxabs) : 0u;
    const float4 z4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
        const uint32_t v = list[i];
        const unsigned long long bit = 1ull << (v & 63u);
        if (accum[8 * (size_t)v + (PACKED ? 3 : 6)] == 0) {   // only the retracted layer was here
            atomicAnd(occ_bits + (v >> 6), ~bit);
            albedo_occ[v] = z4;
            normal[v] = z4;
            level0[l0_texel(v, n)] = z4;
        } else {
            atomicOr(occ_bits + (v >> 6), bit);
            resolve_voxel<PACKED>(accum, v, albedo_occ, normal, maxabs, redo);
        }
    }
}

__global__ void __launch_bounds__(256) k_dyn_occ_list(const unsigned long long* __restrict__ bits, size_t nwords,
                                                      uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    list_block_words(w < nwords ? bits[w] : 0ull, w, list, count);
}

// packed records -> the seven-atomic layout, in place: k1_gather's unpack, k1_restore's store
__global__ void __launch_bounds__(256) k_dyn_unpack(const uint32_t* __restrict__ list, const uint32_t* __restrict__ n_list,
                                                    long long* __restrict__ accum) {
    const uint32_t cnt = *n_list;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < cnt; i += gridDim.x * 256) {
        longlong2* a = (longlong2*)(accum + 8 * (size_t)list[i]);
        const longlong2 p0 = a[0], p1 = a[1];
        long long s[6];
        unpack_sums(p0.x, s[0], s[1]);
        unpack_sums(p0.y, s[2], s[3]);
        unpack_sums(p1.x, s[4], s[5]);
        a[0] = make_longlong2(s[0], s[1]);
        a[1] = make_longlong2(s[2], s[3]);
        a[2] = make_longlong2(s[4], s[5]);
        a[3] = make_longlong2(p1.y, 0);
    }
}

// `bytes` of *p with the first `keep` bytes preserved (the static scene's triangles)
vct_status grow_keeping(vct_ctx* c, float4*& p, size_t& cap, size_t bytes, size_t keep) {
    if (cap >= bytes) return VCT_OK;
    float4* np = nullptr;
    hipError_t e = hipMalloc((void**)&np, bytes);
    if (e != hipSuccess) return lhip(c, e, "hipMalloc mesh");
    if (p && keep) e = hipMemcpyAsync(np, p, keep, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // nothing reads the old array any more
    if (e != hipSuccess) { (void)hipFree(np); return lhip(c, e, "mesh copy"); }
    if (p) (void)hipFree(p);
    p = np;
    cap = bytes;
    return VCT_OK;
}

}  // namespace
}  // namespace vct
