/*
 * vct_env.h — the environment-map sky: an additive extension of include/vct.h (which includes
 * this file; VCT_ABI_VERSION stays 1).
 *
 * vct_sky.h and vct_sky_view.h show the sky through the transmittance of K4's own cones, but
 * the sky they show is three colours blended by one cosine.  This extension puts an image in
 * its place: the context keeps one HDR map with its prefiltered mip chain, Env(d, tau) looks it
 * up by direction and aperture, and four calls mirror the four vct_sky calls argument for
 * argument with a vct_env_sky record where those take a vct_sky.  The march, the receivers,
 * the cone sets, the planes, the counters and the state rules are the sky calls'; only the
 * colour differs.  include/vct_spec.h "environment sky" has the exact arithmetic.
 *
 * The map is OCTAHEDRAL: one square image of S x S RGBA32F texels, S a power of two, with no
 * faces, no transcendental in the lookup and an exact seam rule.  A unit direction e (in map
 * space) lies at p = (e.x, e.y) / (|e.x| + |e.y| + |e.z|) for e.z >= 0 and at the fold of that
 * point over the diamond |p.x| + |p.y| = 1 for e.z < 0; texel (x, y) has its centre at
 * p = ((x + 0.5) * 2 / S - 1, (y + 0.5) * 2 / S - 1), so row 0 is p.y = -1.  Only rgb is used.
 *
 * They live in their own header for the reason vct_sky.h does: vct.h's text is the list of
 * symbols every implementation of the boundary exports, and these are implemented by the HIP
 * library only.
 *
 * Call order:  vct_set_env (any time) ... -> vct_build_mips [-> vct_inject_env | vct_inject_sky]
 *              [-> vct_inject_bounces] -> vct_trace* [-> vct_env_cones_device]
 *              [-> vct_env_specular_device] -> vct_composite_* [-> vct_env_background_device]
 */
#ifndef VCT_ENV_H
#define VCT_ENV_H

#ifdef __cplusplus
extern "C" {
#endif

#define VCT_ENV_MAX_DIM 2048u   /* the largest S */

/* The per-call record; read during the call, not kept in the context.  Input rule: every
 * component of frame finite and its rows orthonormal to VCT_GBUF_ORTHO_EPS = 2^-20 (the
 * camera's rule of the "G-buffer input rule", dot products in double); scale finite, sign bit
 * clear (-0.0f is refused) and <= VCT_ENV_TEXEL_LIMIT.  Anything else is VCT_EINVAL, with
 * nothing written and no state changed. */
typedef struct vct_env_sky {
    float frame[3][3];   /* world -> map rows; e_c = dot3(frame[c], d)          */
    float scale;         /* intensity; finite, sign bit clear, <= 2^52           */
} vct_env_sky;

/* The context's map: host_oct4 = size x size RGBA float texels, row 0 = p.y = -1; size a power
 * of two in 1 .. VCT_ENV_MAX_DIM.  Every texel's r, g and b must be finite, have a clear sign
 * bit (-0.0f is refused) and be <= VCT_ENV_TEXEL_LIMIT = 2^52 (alpha is carried and never
 * read).  Anything else -- a size that is no power of two or too large, NULL host_oct4 with
 * size > 0, a bad texel -- is VCT_EINVAL, and the previous map is kept.  On success the map is
 * uploaded and its mip chain (level j: (size >> j)^2 texels, j = 0 .. lg size, each texel
 * ((a00 + a10) + (a01 + a11)) * 0.25f of its 2 x 2 children) is built on the device; the
 * pyramid belongs to the context and replaces the previous one.  size 0 clears it (host_oct4 is
 * not read).  Synchronous like vct_set_textures: it waits for the ctx stream, so a call queued
 * before it has finished with the previous map when that is released, and host_oct4 may be
 * freed on return.  On a vct_create_multi context the map lives on device 0. */
vct_status vct_set_env(vct_ctx* ctx, const float* host_oct4, uint32_t size);

/* size of the context's map, 0 when none is set (or ctx is NULL) */
uint32_t vct_env_size(const vct_ctx* ctx);

/* host_rgba receives level `level` of the pyramid: (size >> level)^2 x 4 floats, row 0 first.
 * VCT_ESTATE without a map; VCT_EINVAL for NULL host_rgba or level > lg size.  Synchronous. */
vct_status vct_env_download_level(vct_ctx* ctx, uint32_t level, float* host_rgba);

/* One lookup per lane: dir_tau4 = device [count][4] float (d.xyz, tau), out4 = device
 * [count][4] float receives (Env(d, tau).rgb, m), m the level of "environment sky" step 3.
 * Contents are device data, never a status: any direction (zero, NaN, infinite) and any tau
 * have a defined result.  Needs a map (VCT_ESTATE otherwise) and no grid state.  VCT_EINVAL,
 * with nothing written: a record that breaks the input rule, NULL env, NULL or misaligned
 * (16 bytes) dir_tau4 / out4 with count > 0, count > 2^31 - 1.  count 0 is VCT_OK and launches
 * nothing.  Queued on the ctx stream; never waits for the device. */
vct_status vct_env_lookup_device(vct_ctx* ctx, const vct_env_sky* env, const float* dir_tau4, uint32_t count,
                                 float* out4);

/* vct_sky_cones_device with Env(d_k, tau_set) for Sky(d_k): tau_set = VCT_TAN30 for 1 and 9
 * cones, VCT_TAN20 for 16.  Every argument, alignment, NULL and state rule, the counter and the
 * multi-device behaviour are that call's; VCT_ESTATE also when the context has no map. */
vct_status vct_env_cones_device(vct_ctx* ctx, const float* pos4, const float* nrm4,
                                uint32_t width, uint32_t height, const vct_env_sky* env,
                                float* sky4, float* diffuse4_inout, unsigned long long* cone_steps);

/* vct_inject_sky with that Sk.  It shares vct_inject_sky's once-per-level-0 arm: one of the
 * two, once, before vct_inject_bounces on that level 0; VCT_ESTATE otherwise, and without a
 * map.  Every new level 0 re-arms it. */
vct_status vct_inject_env(vct_ctx* ctx, const vct_env_sky* env);

/* vct_sky_specular_device with S_c = T * Env_c(r, tau), tau the pixel's clamped aperture: a
 * rough pixel reflects a blurred sky.  Otherwise that call; VCT_ESTATE also without a map. */
vct_status vct_env_specular_device(vct_ctx* ctx, const float* pos4, const float* nrm4, const float* alb4,
                                   uint32_t width, uint32_t height, const float eye[3], const vct_env_sky* env,
                                   float* skyspec4, float* spec4_inout, unsigned long long* cone_steps);

/* vct_sky_background_device with Env(d, 0) for Sky(d).  Needs a map (VCT_ESTATE otherwise) and
 * no grid state. */
vct_status vct_env_background_device(vct_ctx* ctx, const vct_camera* cam, const float* pos4,
                                     uint32_t width, uint32_t height, const vct_env_sky* env,
                                     float* linear4_inout, uint32_t* rgba8_inout);

#ifdef __cplusplus
}
#endif
#endif /* VCT_ENV_H */
