// vct_sky.hip — the gradient sky: sky light (include/vct_sky.h; the arithmetic is
// include/vct_spec.h "sky light") and the sky in view (include/vct_sky_view.h; "sky in view").
//
//   vct_sky_cones_device     the context's diffuse cone set marched through the alpha of the
//                            pyramid for every pixel, each cone weighting the sky colour of its
//                            direction by the transmittance it ends with.
//   vct_inject_sky           the same for the bounce sources of a voxelization: vct_bounce.hip
//                            keeps the sources as a materialised G-buffer in which every aligned
//                            8x8 block holds 64 neighbouring sources, so the frame kernel runs on
//                            it unchanged; then k_bounce_add_plane (vct_bounce.hip), level 0 +=
//                            A * Sk at every source, and K3.
//   vct_sky_specular_device  the sky in the specular cone of every pixel.
//   vct_sky_background_device  the sky behind the scene.
//
// The kernels, their launchers and the bodies of the four calls are vct_sky_march.h's, shared
// with the environment-map sky (vct_env.hip); this unit brings the colour source: Sky(d), the
// three-colour gradient about `up`, with its input rule.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <string>
#include "vct_internal.h"
#include "vct_light_terms.h"
#include "vct_sky_march.h"

namespace vct {
namespace {

static_assert(sizeof(vct_sky) == 48, "vct_sky is 12 floats (include/vct_sky.h)");

// the constants of Sky(d): up_n and the three colours
struct SkyGradient {
    float ux, uy, uz;
    float zr, zg, zb, hr, hg, hb, gr, gg, gb;

    __device__ __forceinline__ void color(float dx, float dy, float dz, float /*tau*/, float& r, float& g, float& b) const {
        const float u = dot3(dx, dy, dz, ux, uy, uz);
        const float s_up = fminf(fmaxf(u, 0.0f), 1.0f), s_dn = fminf(fmaxf(-u, 0.0f), 1.0f);
        r = (hr + (zr - hr) * s_up) + (gr - hr) * s_dn;
        g = (hg + (zg - hg) * s_up) + (gg - hg) * s_dn;
        b = (hb + (zb - hb) * s_up) + (gb - hb) * s_dn;
    }
};

// the input rule of vct_spec.h "sky light": up by the K2 direction rule, the colours by the K2
// colour rule; fills s, or sets the error and returns its status
vct_status prepare_sky(vct_ctx* c, const char* what, const vct_sky& in, SkyGradient& s) {
    const auto refuse = [&](const char* bad) { return lfail(c, VCT_EINVAL, std::string(what) + ": " + bad); };
    const float ux = in.up[0], uy = in.up[1], uz = in.up[2];
    const float len = sqrtf((ux * ux + uy * uy) + uz * uz);
    if (!(len > 0.0f) || !std::isfinite(len)) return refuse("zero or non-finite up");
    if (const char* bad = check_color(in.zenith)) return refuse(bad);
    if (const char* bad = check_color(in.horizon)) return refuse(bad);
    if (const char* bad = check_color(in.ground)) return refuse(bad);
    s.ux = ux / len; s.uy = uy / len; s.uz = uz / len;
    s.zr = in.zenith[0]; s.zg = in.zenith[1]; s.zb = in.zenith[2];
    s.hr = in.horizon[0]; s.hg = in.horizon[1]; s.hb = in.horizon[2];
    s.gr = in.ground[0]; s.gg = in.ground[1]; s.gb = in.ground[2];
    return VCT_OK;
}

std::atomic<int> g_sky_force64{0};        // vct_debug_sky: every grid takes the 64-bit path
std::atomic<int> g_sky_view_force64{0};   // vct_debug_sky_view: the same for the specular march

}  // namespace
}  // namespace vct

using namespace vct;

extern "C" vct_status vct_sky_cones_device(vct_ctx* c, const float* pos4, const float* nrm4, uint32_t w, uint32_t h,
                                           const vct_sky* sky, float* sky4, float* diffuse4_inout,
                                           unsigned long long* cone_steps) {
    if (!c) return VCT_EINVAL;
    return cones_call<SkyGradient>(c, "sky_cones", "sky", sky, prepare_sky, g_sky_force64, &c->sky_path, pos4, nrm4, w, h,
                                   sky4, diffuse4_inout, cone_steps);
}

extern "C" vct_status vct_inject_sky(vct_ctx* c, const vct_sky* sky) {
    if (!c) return VCT_EINVAL;
    return inject_call<SkyGradient>(c, "inject_sky", "sky", sky, prepare_sky, g_sky_force64, &c->sky_path,
                                    "inject_sky twice on one level 0 (inject or upload a new one first)", c->sky_profile);
}

extern "C" vct_status vct_sky_specular_device(vct_ctx* c, const float* pos4, const float* nrm4, const float* alb4,
                                              uint32_t w, uint32_t h, const float* eye, const vct_sky* sky,
                                              float* skyspec4, float* spec4_inout, unsigned long long* cone_steps) {
    if (!c) return VCT_EINVAL;
    return specular_call<SkyGradient>(c, "sky_specular", "sky", sky, prepare_sky, g_sky_view_force64, &c->sky_view_path,
                                      pos4, nrm4, alb4, w, h, eye, skyspec4, spec4_inout, cone_steps);
}

extern "C" vct_status vct_sky_background_device(vct_ctx* c, const vct_camera* cam, const float* pos4, uint32_t w,
                                                uint32_t h, const vct_sky* sky, float* linear4_inout,
                                                uint32_t* rgba8_inout) {
    if (!c) return VCT_EINVAL;
    return background_call<SkyGradient>(c, "sky_background", "sky", sky, prepare_sky, cam, pos4, w, h, linear4_inout,
                                        rgba8_inout);
}

// Test and tool hook (not part of the public headers).  force64 >= 0: nonzero sends every
// grid's sky march through the 64-bit-address path that 1024^3 takes (process-wide).
// profile >= 0 (with a context): nonzero times the stages of the following vct_inject_sky
// calls with events (the call then waits for its last stage).  ms3 (nullable) receives the
// march, add and K3 times of the last timed vct_inject_sky.
extern "C" int vct_debug_sky(vct_ctx* c, int force64, int profile, float* ms3) {
    if (force64 >= 0) g_sky_force64.store(force64 ? 1 : 0);
    if (c && profile >= 0) c->sky_profile = profile != 0;
    if (c && ms3)
        for (int i = 0; i < 3; ++i) ms3[i] = c->sky_ms[i];
    return 0;
}

// The address path the context's last sky march was launched with: 32 (buffer resources), 64
// (64-bit addresses), 0 before the first one.
extern "C" int vct_debug_sky_path(const vct_ctx* c) { return c ? c->sky_path : -1; }

// Test and tool hook (not part of the public headers).  force64 >= 0: nonzero sends every
// grid's specular sky march through the 64-bit-address path that 1024^3 takes (process-wide).
extern "C" int vct_debug_sky_view(int force64) {
    if (force64 >= 0) g_sky_view_force64.store(force64 ? 1 : 0);
    return 0;
}

// The address path the context's last specular sky march was launched with: 32 (buffer
// resources), 64 (64-bit addresses), 0 before the first one.
extern "C" int vct_debug_sky_view_path(const vct_ctx* c) { return c ? c->sky_view_path : -1; }
