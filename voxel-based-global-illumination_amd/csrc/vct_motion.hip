// vct_motion.hip — object motion (include/vct_motion.h; include/vct_spec.h "object motion"):
// the previous-position plane of vct_temporal_accumulate_device, and the normal plane that goes
// with it, from the object set's poses.  Image space: no grid, no pyramid.
//
//   k_obj_scatter_poses  the set remembers its poses: poses[ids[j]] = the update's pose j, one
//                        lane per word (vct_objects.hip launches it from objects_move).
//   kmotion_flags        one lane per object: hidden in the snapshot, unmoved (the twelve floats
//                        the transform rule reads are the snapshot's in every bit) or moved.  The
//                        pixel kernel then reads 4 bytes per object, not two 80-byte poses.
//   kmotion<NRM>         one lane per pixel, in row-major order (every plane is read and written
//                        once, fully coalesced).  A wave whose ballot finds no lane on the set
//                        copies: motion4 = (pos4.xyz, 1), prev_nrm4 = nrm4.  Otherwise it serves
//                        the distinct objects its lanes hold one at a time: the first pending
//                        lane's id is made wave-uniform, the search over `first` (at most 12
//                        steps for 4 096 objects), the object's range, flag and the snapshot's
//                        matrix are then uniform too and stay in scalar registers; the lanes in
//                        that range transform their triangle's three object-space vertices.
//   kmotion_sum          one block: the frame's four stats from one word per wave (no atomics,
//                        as ktemporal_sum).
//
// A frame is bound by its planes: 44 bytes a pixel (76 with the normal planes), plus 36 bytes of
// vertices and 12 of indices on a moved object's pixels, which neighbouring lanes share.
#include <hip/hip_runtime.h>
#include <cstring>
#include <string>
#include "vct_internal.h"

namespace vct {
namespace {

struct MotionPose {      // vct_object_pose as the kernels read it
    float m[16];
    uint32_t visible, reserved[3];
};
static_assert(sizeof(MotionPose) == 80 && sizeof(vct_object_pose) == 80, "vct_object_pose is 80 bytes");

enum { kWasHidden = 0u, kUnmoved = 1u, kMoved = 2u };                 // kmotion_flags' word
enum { kBackground = 0, kStill = 1, kMovedPx = 2, kAppeared = 3 };    // a pixel's class

__global__ void __launch_bounds__(256) k_obj_scatter_poses(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ src,
                                                           uint32_t n, uint32_t* __restrict__ dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // word i of the update's 20 n
    if (i >= 20u * n) return;
    const uint32_t j = i / 20u, w = i - 20u * j;
    dst[20u * (size_t)ids[j] + w] = src[i];
}

__global__ void __launch_bounds__(256) kmotion_flags(const MotionPose* __restrict__ cur, const MotionPose* __restrict__ prev,
                                                     uint32_t n_objects, uint32_t* __restrict__ flags) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_objects) return;
    uint32_t f = kWasHidden;
    if (prev[o].visible != 0u) {
        f = kUnmoved;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if ((j & 3) != 3 && __float_as_uint(cur[o].m[j]) != __float_as_uint(prev[o].m[j])) f = kMoved;
    }
    flags[o] = f;
}

struct MotionK {
    const float4 *pos, *nrm;                 // nrm: with pnrm only
    const uint32_t* tri;
    const float2* bary;
    const MotionPose *cur, *prev;
    const uint32_t *first, *flags;           // [n_objects + 1], [n_objects]
    const float* vpos;                       // the set's object-space positions
    const uint32_t* vidx;                    // [3 n_set]
    float4 *motion, *pnrm;
    uint32_t* wstat;                         // [waves]: still | moved << 8 | appeared << 16 (each <= 64); nullable
    uint32_t npix, n_static, n_set, n_objects;
};

// the transform rule (vct_spec.h "dynamic objects"): one rounding per operation, no fma
__device__ __forceinline__ float xform_row(float a, float b, float c, float d, float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)), __fmul_rn(c, z)), d);
}

// vertex v (object space) under m -> out
__device__ __forceinline__ void xform(const float* __restrict__ m, const float v[3], float out[3]) {
    out[0] = xform_row(m[0], m[4], m[8], m[12], v[0], v[1], v[2]);
    out[1] = xform_row(m[1], m[5], m[9], m[13], v[0], v[1], v[2]);
    out[2] = xform_row(m[2], m[6], m[10], m[14], v[0], v[1], v[2]);
}

// e1 x e2 of the transformed triangle, unit() of "shading attributes": false where undefined
__device__ __forceinline__ bool face_unit(const float p[3][3], float n[3]) {
    const float e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
    const float e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float sq = dot3(nx, ny, nz, nx, ny, nz);
    const float l = sqrtf(sq);
    n[0] = nx / l; n[1] = ny / l; n[2] = nz / l;
    return sq > 0.0f && sq < __builtin_inff();
}

template <bool NRM>
__global__ void __launch_bounds__(256) kmotion(const MotionK k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool in = i < k.npix;
    float4 P = make_float4(0.0f, 0.0f, 0.0f, 0.0f), N = P;
    uint32_t id = 0;
    if (in) {
        P = k.pos[i];
        id = k.tri[i];
        if (NRM) N = k.nrm[i];
    }
    const bool valid = in && P.w != 0.0f;
    float4 M = make_float4(P.x, P.y, P.z, 1.0f), Q = N;     // the static record
    int cls = valid ? kStill : kBackground;
    if (!valid) M = Q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool dyn = valid && id >= k.n_static;
    if (__builtin_amdgcn_ballot_w64(dyn) != 0ull) {          // else: the pure copy path
        const uint32_t t = id - k.n_static;                  // the set's triangle, where dyn
        bool pending = dyn && t < k.n_set;
        if (dyn && !pending) { M = make_float4(0.0f, 0.0f, 0.0f, 0.0f); cls = kAppeared; }   // names no triangle
        unsigned long long todo;
        while ((todo = __builtin_amdgcn_ballot_w64(pending)) != 0ull) {
            // the first pending lane's triangle, wave-uniform from here on
            const int l0 = (int)__builtin_ctzll(todo);
            const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)t, l0);
            uint32_t lo = 0, hi = k.n_objects;               // the last object with first[o] <= t0
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (k.first[mid] <= t0) lo = mid; else hi = mid;
            }
            const uint32_t f0 = k.first[lo], f1 = k.first[lo + 1], flag = k.flags[lo];
            const bool mine = pending && t >= f0 && t < f1;
            if (flag == kWasHidden) {
                if (mine) { M = make_float4(0.0f, 0.0f, 0.0f, 0.0f); cls = kAppeared; }
            } else if (flag == kMoved) {
                const float* pm = k.prev[lo].m;
                const float* cm = k.cur[lo].m;
                if (mine) {
                    const float2 b = k.bary[i];
                    float v[3][3], p[3][3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float* src = k.vpos + 3 * (size_t)k.vidx[3 * (size_t)t + j];
                        v[j][0] = src[0]; v[j][1] = src[1]; v[j][2] = src[2];
                        xform(pm, v[j], p[j]);
                    }
                    float q[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) q[a] = fmaf(b.y, p[2][a] - p[0][a], fmaf(b.x, p[1][a] - p[0][a], p[0][a]));
                    const float inf = __builtin_inff();
                    if (fabsf(q[0]) < inf && fabsf(q[1]) < inf && fabsf(q[2]) < inf) {
                        M = make_float4(q[0], q[1], q[2], 1.0f);
                        cls = kMovedPx;
                    } else {
                        M = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        cls = kAppeared;
                    }
                    if (NRM) {
                        float np[3], nc[3], c[3][3];
                        const bool okp = face_unit(p, np);
#pragma unroll
                        for (int j = 0; j < 3; ++j) xform(cm, v[j], c[j]);
                        const bool okc = face_unit(c, nc);
                        if (okp && okc) {
                            const bool flip = dot3(nc[0], nc[1], nc[2], N.x, N.y, N.z) < 0.0f;
                            Q = flip ? make_float4(-np[0], -np[1], -np[2], 0.0f) : make_float4(np[0], np[1], np[2], 0.0f);
                        }
                    }
                }
            }
            pending = pending && !mine && (int)(threadIdx.x & 63u) != l0;   // (lane l0 is always `mine`: first is monotone)
        }
    }
    if (in) {
        k.motion[i] = M;
        if (NRM) k.pnrm[i] = Q;
    }
    if (k.wstat) {                               // wave-uniform: one word per wave, summed by kmotion_sum
        const uint32_t ns = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == kStill));
        const uint32_t nm = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == kMovedPx));
        const uint32_t na = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == kAppeared));
        if ((threadIdx.x & 63u) == 0u && in) k.wstat[i >> 6] = ns | nm << 8 | na << 16;   // (a wave past the frame has no word)
    }
}

// one block: the sums of the waves' words (each field <= 64, so a byte each)
__global__ void __launch_bounds__(1024) kmotion_sum(const uint32_t* __restrict__ wstat, uint32_t waves,
                                                    uint32_t* __restrict__ stats) {
    __shared__ uint32_t part[3][16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t ns = 0, nm = 0, na = 0;
    for (uint32_t i = (uint32_t)tid; i < waves; i += 1024u) {
        const uint32_t ws = wstat[i];
        ns += ws & 0xffu;
        nm += (ws >> 8) & 0xffu;
        na += (ws >> 16) & 0xffu;
    }
    ns = wave_sum_u32(ns);
    nm = wave_sum_u32(nm);
    na = wave_sum_u32(na);
    if (lane == 0) { part[0][wave] = ns; part[1][wave] = nm; part[2][wave] = na; }
    __syncthreads();
    if (tid == 0) {
        ns = nm = na = 0;
        for (int j = 0; j < 16; ++j) { ns += part[0][j]; nm += part[1][j]; na += part[2][j]; }
        stats[0] = ns + nm + na;
        stats[1] = ns;
        stats[2] = nm;
        stats[3] = na;
    }
}

// ---- host side --------------------------------------------------------------------------
inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

const char* check_args(const vct_motion_args& a) {
    if (a.width == 0 || a.height == 0 || a.width > 65536 || a.height > 65536 ||
        (uint64_t)a.width * a.height > 0x7fffffffull)
        return "bad frame size";
    if (!a.pos4 || !a.tri_id || !a.bary2 || !a.prev_poses || !a.motion4) return "NULL buffer";
    if ((a.nrm4 == nullptr) != (a.prev_nrm4 == nullptr)) return "nrm4 and prev_nrm4 go together";
    if (!al(a.pos4, 16) || !al(a.nrm4, 16) || !al(a.motion4, 16) || !al(a.prev_nrm4, 16))
        return "float4 buffers must be 16-byte aligned";
    if (!al(a.prev_poses, 16)) return "prev_poses must be 16-byte aligned";
    if (!al(a.bary2, 8)) return "bary2 must be 8-byte aligned";
    if (!al(a.tri_id, 4) || !al(a.stats, 4)) return "uint32 buffers must be 4-byte aligned";
    return nullptr;
}

}  // namespace

void objects_scatter_poses(hipStream_t s, const uint32_t* ids, const void* src, uint32_t n, void* poses) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_obj_scatter_poses, dim3((20u * n + 255u) / 256u), dim3(256), 0, s, ids, (const uint32_t*)src, n,
                       (uint32_t*)poses);
}

}  // namespace vct

using namespace vct;

extern "C" vct_status vct_objects_poses_device(vct_ctx* c, vct_object_pose* out, uint32_t capacity) {
    if (!c) return VCT_EINVAL;
    if (!out || !al(out, 16)) return lfail(c, VCT_EINVAL, "objects_poses_device: out is NULL or not 16-byte aligned");
    if (!objects_live(c)) return lfail(c, VCT_ESTATE, "objects_poses_device without an object set (vct_objects_define first)");
    const Objects& o = c->obj;
    if (capacity < o.n_objects)
        return lfail(c, VCT_EINVAL, "objects_poses_device: capacity " + std::to_string(capacity) + " < n_objects");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    e = hipMemcpyAsync(out, o.poses, sizeof(MotionPose) * (size_t)o.n_objects, hipMemcpyDeviceToDevice, c->stream);
    return e == hipSuccess ? VCT_OK : lhip(c, e, "objects_poses_device");
}

extern "C" vct_status vct_objects_motion_device(vct_ctx* c, const vct_motion_args* a) {
    if (!c || !a) return VCT_EINVAL;
    if (const char* bad = check_args(*a)) return lfail(c, VCT_EINVAL, std::string("objects_motion: ") + bad);
    if (!objects_live(c)) return lfail(c, VCT_ESTATE, "objects_motion without an object set (vct_objects_define first)");
    const Objects& o = c->obj;
    if (a->n_prev != o.n_objects)
        return lfail(c, VCT_EINVAL, "objects_motion: n_prev " + std::to_string(a->n_prev) + " != n_objects");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    MotionK k;
    std::memset(&k, 0, sizeof k);
    k.npix = a->width * a->height;
    const uint32_t waves = (k.npix + 63u) / 64u;
    // scratch of the stream: the objects' flags, then the waves' words; every word read is
    // written by a launch before it
    const size_t flag_bytes = ((size_t)o.n_objects * 4 + 255) & ~(size_t)255;
    void* sp = nullptr;
    if ((e = k4_scratch(c, kScMotion, flag_bytes + (a->stats ? (size_t)waves * 4 : 0), &sp, nullptr)) != hipSuccess)
        return lhip(c, e, "objects_motion: scratch");
    uint32_t* flags = (uint32_t*)sp;
    k.pos = (const float4*)a->pos4; k.nrm = (const float4*)a->nrm4;
    k.tri = a->tri_id; k.bary = (const float2*)a->bary2;
    k.cur = (const MotionPose*)o.poses; k.prev = (const MotionPose*)a->prev_poses;
    k.first = o.d_first; k.flags = flags;
    k.vpos = o.pos; k.vidx = o.idx;
    k.motion = (float4*)a->motion4; k.pnrm = (float4*)a->prev_nrm4;
    k.wstat = a->stats ? (uint32_t*)((char*)sp + flag_bytes) : nullptr;
    k.n_static = o.n_static; k.n_set = o.n_tri; k.n_objects = o.n_objects;
    hipLaunchKernelGGL(kmotion_flags, dim3((o.n_objects + 255u) / 256u), dim3(256), 0, c->stream, k.cur, k.prev, o.n_objects,
                       flags);
    const dim3 grid((k.npix + 255u) / 256u);
    if (a->prev_nrm4) hipLaunchKernelGGL(kmotion<true>, grid, dim3(256), 0, c->stream, k);
    else hipLaunchKernelGGL(kmotion<false>, grid, dim3(256), 0, c->stream, k);
    if (a->stats) hipLaunchKernelGGL(kmotion_sum, dim3(1), dim3(1024), 0, c->stream, (const uint32_t*)k.wstat, waves, a->stats);
    e = hipGetLastError();
    return e == hipSuccess ? VCT_OK : lhip(c, e, "objects_motion");
}
