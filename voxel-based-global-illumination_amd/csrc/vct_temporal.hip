// vct_temporal.hip — temporal accumulation (include/vct_temporal.h; include/vct_spec.h
// "temporal accumulation").  Image space only: no grid, no pyramid, no other unit's device code.
//
//   ktemporal<NP>   one lane per pixel (8x8 per wave, partial blocks at the right and bottom
//                   edges): previous position -> last frame's pixel coordinates -> four taps in
//                   integers -> the upsample's normal and plane tests -> H = S / W per plane ->
//                   out = H + (cur - H) / k.  NP planes share the reprojection and the tests;
//                   the template keeps their tap sums in registers.
//   ktemporal_sum   one block: the frame's four stats from one word per wave.  No atomics: one
//                   address counted into by every wave of a frame costs more than the kernel
//                   (0.507 against 0.067 ms).
//
// Under coherent motion the four taps of a wave are a 9x9 patch of last frame's pixels that the
// neighbouring waves reread: they are left to L2, the kernel holds no LDS and no barrier, and
// it is bound by the planes it reads and writes (DESIGN 10.9 has the resource table and rate).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "vct_internal.h"
#include "vct_light_terms.h"
#include "vct_view.h"

namespace vct {
namespace {

static_assert(sizeof(vct_temporal_params) == 12, "vct_temporal_params is 3 words (include/vct_temporal.h)");

struct TempK {
    const float4 *pos, *nrm, *motion;        // motion: nullable
    const float4 *ppos, *pnrm;               // read with has_prev only
    const float4* cur[4];
    const float4* hist[4];
    float4* out[4];
    const uint32_t* hlen;
    uint32_t* olen;
    uint32_t* wstat;                         // [waves]: reused | offscreen << 8 | rejected << 16 (each <= 64); nullable
    int w, h, tiles_x, has_prev;
    float ex, ey, ez;                        // last frame's camera (camera_fields)
    float fx, fy, fz, ux, uy, uz, rx, ry, rz, tan_half, aspect;
    float ncos, eps;
    uint32_t max_len;
};

__device__ __forceinline__ bool finite4(const float4 v) {
    const float inf = __builtin_inff();
    return fabsf(v.x) < inf && fabsf(v.y) < inf && fabsf(v.z) < inf && fabsf(v.w) < inf;
}

enum { kBackground = 0, kReused = 1, kOffscreen = 2, kRejected = 3 };

template <int NP>
__global__ void __launch_bounds__(64) ktemporal(const TempK k) {
    const int lane = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / k.tiles_x, tx = (int)blockIdx.x - ty * k.tiles_x;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const bool inframe = x < k.w && y < k.h;
    const size_t i = inframe ? (size_t)y * (size_t)k.w + (size_t)x : 0;
    float4 P = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inframe) P = k.pos[i];
    int cls = kBackground;
    if (inframe && P.w != 0.0f) {
        float4 c[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) c[p] = k.cur[p][i];
        cls = kOffscreen;
        float qx = P.x, qy = P.y, qz = P.z, px = 0.0f, py = 0.0f;
        bool projected = false;
        if (k.has_prev) {
            bool existed = true;
            if (k.motion) {
                const float4 m = k.motion[i];
                qx = m.x; qy = m.y; qz = m.z;
                existed = !(m.w == 0.0f);
            }
            const float vx = qx - k.ex, vy = qy - k.ey, vz = qz - k.ez;
            const float z = dot3(vx, vy, vz, k.fx, k.fy, k.fz);
            if (existed && z > 0.0f) {
                const float a = dot3(vx, vy, vz, k.rx, k.ry, k.rz);
                const float b = dot3(vx, vy, vz, k.ux, k.uy, k.uz);
                const float kx = k.tan_half * k.aspect;
                const float sx = a / (z * kx), sy = b / (z * k.tan_half);
                px = ((sx + 1.0f) * 0.5f) * (float)k.w - 0.5f;
                py = ((1.0f - sy) * 0.5f) * (float)k.h - 0.5f;
                projected = px > -1.0f && px < (float)k.w && py > -1.0f && py < (float)k.h;
            }
        }
        if (projected) {
            cls = kRejected;
            const float4 N = k.nrm[i];
            const int X16 = (int)floorf(px * 16.0f + 0.5f), Y16 = (int)floorf(py * 16.0f + 0.5f);   // -16 .. 16 w
            const int x0 = X16 >> 4, y0 = Y16 >> 4, rx = X16 & 15, ry = Y16 & 15;
            uint32_t W = 0, L = 0xffffffffu;
            float4 s[NP] = {};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int ti = t & 1, tj = t >> 1;
                const int X = x0 + ti, Y = y0 + tj;
                const int bw = (ti ? rx : 16 - rx) * (tj ? ry : 16 - ry);
                if (X < 0 || X >= k.w || Y < 0 || Y >= k.h || bw == 0) continue;
                const size_t q = (size_t)Y * (size_t)k.w + (size_t)X;
                const float4 Pq = k.ppos[q];
                const uint32_t lq = k.hlen[q];
                if (Pq.w == 0.0f || lq == 0u) continue;
                const float4 Nq = k.pnrm[q];
                const float cn = dot3(N.x, N.y, N.z, Nq.x, Nq.y, Nq.z);
                const float d = fabsf(dot3(N.x, N.y, N.z, Pq.x - qx, Pq.y - qy, Pq.z - qz));
                if (!(cn >= k.ncos) || !(d <= k.eps)) continue;
                const float fb = (float)bw;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    const float4 V = k.hist[p][q];
                    if (W == 0) s[p] = make_float4(fb * V.x, fb * V.y, fb * V.z, fb * V.w);
                    else { s[p].x = s[p].x + fb * V.x; s[p].y = s[p].y + fb * V.y; s[p].z = s[p].z + fb * V.z; s[p].w = s[p].w + fb * V.w; }
                }
                W += (uint32_t)bw;
                L = lq < L ? lq : L;
            }
            if (W != 0) {
                const float fw = (float)W;
                bool fin = true;
#pragma unroll
                for (int p = 0; p < NP; ++p) {
                    s[p] = make_float4(s[p].x / fw, s[p].y / fw, s[p].z / fw, s[p].w / fw);
                    fin = fin && finite4(s[p]);
                }
                const uint32_t kk = (L < k.max_len - 1u ? L : k.max_len - 1u) + 1u;
                if (fin && kk >= 2u) {
                    cls = kReused;
                    const float wk = 1.0f / (float)kk;
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        const float4 H = s[p];
                        k.out[p][i] = make_float4(H.x + (c[p].x - H.x) * wk, H.y + (c[p].y - H.y) * wk,
                                                  H.z + (c[p].z - H.z) * wk, H.w + (c[p].w - H.w) * wk);
                    }
                    k.olen[i] = kk;
                }
            }
        }
        if (cls != kReused) {
#pragma unroll
            for (int p = 0; p < NP; ++p) k.out[p][i] = c[p];
            k.olen[i] = 1u;
        }
    } else if (inframe) {
#pragma unroll
        for (int p = 0; p < NP; ++p) k.out[p][i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        k.olen[i] = 0u;
    }
    if (k.wstat) {                               // wave-uniform: one word per wave, summed by ktemporal_sum
        const uint32_t nu = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == kReused));
        const uint32_t no = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == kOffscreen));
        const uint32_t nj = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls == kRejected));
        if (lane == 0) k.wstat[blockIdx.x] = nu | no << 8 | nj << 16;   // valid is their sum
    }
}

// one block: the sums of the waves' words (each field <= 64, so a byte each)
__global__ void __launch_bounds__(1024) ktemporal_sum(const uint32_t* __restrict__ wstat, uint32_t waves,
                                                      uint32_t* __restrict__ stats) {
    __shared__ uint32_t part[3][16];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t nu = 0, no = 0, nj = 0;
    for (uint32_t i = (uint32_t)tid; i < waves; i += 1024u) {
        const uint32_t ws = wstat[i];
        nu += ws & 0xffu;
        no += (ws >> 8) & 0xffu;
        nj += (ws >> 16) & 0xffu;
    }
    nu = wave_sum_u32(nu);
    no = wave_sum_u32(no);
    nj = wave_sum_u32(nj);
    if (lane == 0) { part[0][wave] = nu; part[1][wave] = no; part[2][wave] = nj; }
    __syncthreads();
    if (tid == 0) {
        nu = no = nj = 0;
        for (int j = 0; j < 16; ++j) { nu += part[0][j]; no += part[1][j]; nj += part[2][j]; }
        stats[0] = nu + no + nj;
        stats[1] = nu;
        stats[2] = no;
        stats[3] = nj;
    }
}

// ---- host side --------------------------------------------------------------------------
inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool al4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

const char* check_params(const vct_temporal_params& p) {
    if (!std::isfinite(p.normal_cos) || p.normal_cos < -1.0f || p.normal_cos > 1.0f) return "normal_cos outside [-1, 1]";
    if (!std::isfinite(p.plane_eps) || std::signbit(p.plane_eps)) return "plane_eps not finite or negative";
    if (p.max_len < 1 || p.max_len > VCT_TEMPORAL_MAX_LEN) return "max_len outside 1 .. VCT_TEMPORAL_MAX_LEN";
    return nullptr;
}

const char* check_args(const vct_temporal_args& a) {
    if (a.width == 0 || a.height == 0 || a.width > 65536 || a.height > 65536 ||
        (uint64_t)a.width * a.height > 0x7fffffffull)
        return "bad frame size";
    if (a.n_planes == 0 || a.n_planes > 4) return "n_planes must be 1 .. 4";
    if (!a.pos4 || !a.nrm4 || !a.out_len) return "NULL buffer";
    if (!al16(a.pos4) || !al16(a.nrm4) || !al16(a.motion4)) return "float4 buffers must be 16-byte aligned";
    if (!al4(a.out_len) || !al4(a.stats)) return "uint32 buffers must be 4-byte aligned";
    for (uint32_t p = 0; p < a.n_planes; ++p) {
        if (!a.cur4[p] || !a.out4[p]) return "NULL plane";
        if (!al16(a.cur4[p]) || !al16(a.out4[p])) return "float4 buffers must be 16-byte aligned";
    }
    if (a.prev_cam) {
        const vct_camera& c = *a.prev_cam;
        const float th = tanf(c.zoom_deg * 0.5f * 3.14159265358979f / 180.0f);   // camera_fields' tan_half
        if (!std::isfinite(th) || !(th > 0.0f)) return "prev_cam: tan(zoom / 2) is not finite and > 0";
        if (!finite3(c.position) || !finite3(c.front) || !finite3(c.up) || !finite3(c.right))
            return "prev_cam: non-finite position or vector";
        if (!a.prev_pos4 || !a.prev_nrm4 || !a.hist_len) return "prev_cam without a previous G-buffer or hist_len";
        if (!al16(a.prev_pos4) || !al16(a.prev_nrm4)) return "float4 buffers must be 16-byte aligned";
        if (!al4(a.hist_len)) return "uint32 buffers must be 4-byte aligned";
        for (uint32_t p = 0; p < a.n_planes; ++p) {
            if (!a.hist4[p]) return "prev_cam without hist4";
            if (!al16(a.hist4[p])) return "float4 buffers must be 16-byte aligned";
        }
    }
    // a history is read at other pixels than the one written: it may not be an output.  The
    // rule is the pointers', whether or not this call reads them.
    for (uint32_t p = 0; p < a.n_planes; ++p)
        for (uint32_t q = 0; q < a.n_planes; ++q)
            if (a.hist4[q] && a.out4[p] == a.hist4[q]) return "out4 aliases hist4";
    if (a.hist_len && a.out_len == a.hist_len) return "out_len aliases hist_len";
    return nullptr;
}

template <int NP>
void launch(const TempK& k, uint32_t waves, hipStream_t s) {
    hipLaunchKernelGGL(ktemporal<NP>, dim3(waves), dim3(64), 0, s, k);
}

}  // namespace
}  // namespace vct

using namespace vct;

extern "C" vct_status vct_temporal_default_params(const vct_ctx* c, vct_temporal_params* out) {
    if (!c || !out) return VCT_EINVAL;
    out->normal_cos = VCT_MIXED_NORMAL_COS;
    out->plane_eps = c->cfg.extent / (float)c->cfg.n;
    out->max_len = VCT_TEMPORAL_DEFAULT_LEN;
    return VCT_OK;
}

extern "C" vct_status vct_temporal_accumulate_device(vct_ctx* c, const vct_temporal_args* a,
                                                     const vct_temporal_params* p) {
    if (!c || !a || !p) return VCT_EINVAL;
    if (const char* bad = check_params(*p)) return lfail(c, VCT_EINVAL, std::string("temporal_accumulate: ") + bad);
    if (const char* bad = check_args(*a)) return lfail(c, VCT_EINVAL, std::string("temporal_accumulate: ") + bad);
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return lhip(c, e, "hipSetDevice");
    TempK k;
    std::memset(&k, 0, sizeof k);
    k.pos = (const float4*)a->pos4; k.nrm = (const float4*)a->nrm4; k.motion = (const float4*)a->motion4;
    k.has_prev = a->prev_cam ? 1 : 0;
    if (a->prev_cam) {
        camera_fields(k, a->prev_cam, a->width, a->height);
        k.ex = a->prev_cam->position[0]; k.ey = a->prev_cam->position[1]; k.ez = a->prev_cam->position[2];
        k.ppos = (const float4*)a->prev_pos4; k.pnrm = (const float4*)a->prev_nrm4;
        k.hlen = a->hist_len;
    }
    k.w = (int)a->width; k.h = (int)a->height;
    for (uint32_t q = 0; q < a->n_planes; ++q) {
        k.cur[q] = (const float4*)a->cur4[q];
        k.hist[q] = a->prev_cam ? (const float4*)a->hist4[q] : nullptr;
        k.out[q] = (float4*)a->out4[q];
    }
    k.olen = a->out_len;
    k.tiles_x = (int)((a->width + 7) / 8);
    k.ncos = p->normal_cos; k.eps = p->plane_eps; k.max_len = p->max_len;
    const uint32_t waves = (uint32_t)k.tiles_x * ((a->height + 7) / 8);
    if (a->stats) {   // scratch of the stream: every word read is written by the launch before it
        void* sp = nullptr;
        if ((e = k4_scratch(c, kScTemporal, (size_t)waves * 4, &sp, nullptr)) != hipSuccess)
            return lhip(c, e, "temporal_accumulate: scratch");
        k.wstat = (uint32_t*)sp;
    }
    switch (a->n_planes) {
        case 1: launch<1>(k, waves, c->stream); break;
        case 2: launch<2>(k, waves, c->stream); break;
        case 3: launch<3>(k, waves, c->stream); break;
        default: launch<4>(k, waves, c->stream); break;
    }
    if (a->stats)
        hipLaunchKernelGGL(ktemporal_sum, dim3(1), dim3(1024), 0, c->stream, (const uint32_t*)k.wstat, waves, a->stats);
    e = hipGetLastError();
    return e == hipSuccess ? VCT_OK : lhip(c, e, "temporal_accumulate");
}
