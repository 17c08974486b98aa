/*
 * vct_fog.h — volumetric fog: an additive extension of include/vct.h (which includes this
 * file; VCT_ABI_VERSION stays 1).
 *
 * Every other term of the frame is evaluated at the G-buffer's hit point.  The functions here
 * show light in the space between the eye and that point: a homogeneous medium that scatters
 * the lights of a list (and, weighted by `ambient`, the cone-traced indirect light) toward the
 * viewer.  vct_build_fog fills a scatter volume of (n >> level)^3 cells from the radiance
 * pyramid -- the visibility of a light at a cell centre is the alpha march of vct_shadow.h --
 * vct_fog_rays_device turns a G-buffer into view-ray segments, vct_fog_march_device integrates
 * the volume along them into (F.rgb, T) per pixel, and vct_fog_apply_device puts
 * rgb = rgb * T + F on a composite's linear frame.  include/vct_spec.h "volumetric fog" has
 * the exact arithmetic.
 *
 * The opacity of one march step is a = min(sigma * ds, 1), linear in the step length, and the
 * phase function is isotropic: no transcendental enters the march, so the numpy restatement
 * under tests/ is exact and every GPU comparison is bit for bit.  An exponential transmittance
 * and an anisotropic phase are deliberately left out.
 *
 * They live in their own header for the reason vct_bounce.h, vct_lights.h, vct_shadow.h,
 * vct_emission.h and vct_sky.h do: vct.h's text is the list of symbols every implementation of
 * the boundary exports, and these are implemented by the HIP library only.
 *
 * Call order:  ... -> vct_build_mips [-> vct_inject_sky] [-> vct_inject_bounces]
 *              -> vct_build_fog -> vct_trace* -> vct_composite_*
 *              -> vct_fog_rays_device -> vct_fog_march_device -> vct_fog_apply_device
 *
 * The vct_fog record and the light list are read during the call; they are not kept.
 */
#ifndef VCT_FOG_H
#define VCT_FOG_H

#ifdef __cplusplus
extern "C" {
#endif

/* The medium.  Input rule (anything else is VCT_EINVAL, with nothing written and no state
 * changed):
 *   density  extinction per world unit: finite, sign bit clear, <= VCT_FOG_DENSITY_LIMIT; the
 *            kernels use sigma_v = (density * E) / (float)n, the extinction per voxel length
 *            (float32, in that order), which must be finite
 *   albedo   single-scattering albedo: each finite and in [0, 1]; -0.0f is refused
 *   ambient  weight of the indirect term: finite and >= 0; 0 switches the term off (no K4
 *            launch happens)
 *   level    one cell = 2^level voxels: 1 <= level and (n >> level) >= 4
 *   step     march step in cells: in [0.25, 4] */
typedef struct vct_fog {
    float density;
    float albedo[3];
    float ambient;
    uint32_t level;
    float step;
} vct_fog;

/* Header defaults of the fields a host usually leaves alone. */
#define VCT_FOG_DEFAULT_ALBEDO  0.9f
#define VCT_FOG_DEFAULT_AMBIENT 0.0f
#define VCT_FOG_DEFAULT_LEVEL   2u
#define VCT_FOG_DEFAULT_STEP    1.0f
#define VCT_FOG_DEFAULT_TAN     0.1f     /* aperture of a light's visibility cone */

/* The scatter volume: m^3 cells of float4, m = n >> fog->level, owned by the context
 * (16 m^3 bytes; allocated at the first build, reused while m is unchanged, freed with the
 * context).  Cell (i, j, k) holds, for its centre x_c = (i + 1/2, j + 1/2, k + 1/2) 2^level,
 *     S = albedo * (VCT_FOG_PHASE * sum_j C_j att_j(x_c) V_j(x_c) + ambient * A(x_c))
 * in .rgb and +0 in .w.  att_j is the range and spot-cone factor of vct_lights.h at x_c
 * without the n.l cosine (1 for a directional light); V_j is the visibility of vct_shadow.h's
 * cone from x_c itself toward the light with aperture tan_half[j] clamped to
 * [VCT_SPEC_TAU_MIN, VCT_SPEC_TAU_MAX]; A = (I+ + I-) / 2 with I the rgb of K4's diffuse plane
 * for a record at x_c with normal +y / -y (only when ambient > 0 and n_diffuse > 0).
 * lights / n_lights follow vct_inject_lights' input rule; every tan_half[j] must be finite
 * and > 0 (there is no hard walk in a medium).  n_lights = 0 with ambient = 0 builds an
 * all-zero volume, which is valid: the march then only attenuates.
 * Needs a voxelization and built mips (VCT_ESTATE otherwise).  The volume belongs to the
 * pyramid it was built from: any later voxelization, dynamic update, inject, upload, load or
 * vct_build_mips makes it stale.  The step tables are the context's (vct_shadow.h): a fog
 * build, a sky call and a shadow call of one context run in the order they were made.
 * Queued on the ctx stream; never waits for the device.  On a vct_create_multi context
 * device 0 builds and keeps the volume. */
vct_status vct_build_fog(vct_ctx* ctx, const vct_fog* fog, const vct_light* lights, uint32_t n_lights,
                         const float* tan_half);

/* The cell count m of the current volume / a copy of it as m^3 x 4 floats in linear z, y, x
 * order (waits for the ctx stream).  VCT_ESTATE without a current volume. */
vct_status vct_fog_dims(const vct_ctx* ctx, uint32_t* m);
vct_status vct_download_fog(vct_ctx* ctx, float* host_rgba);

/* The view-ray segment of every pixel: ray4 = device [height][width][4] float (16-byte
 * aligned) receives (d.xyz, len) in voxel units.
 *   valid pixel (pos.w != 0): the segment from the eye to the pixel's position, d unit.
 *   background pixel: with cam, the direction of the pixel's primary ray (the G-buffer
 *     caster's) and len = +inf; with cam NULL, +0 in all four channels.
 *   a ray that is not a ray (len 0 or not finite, a non-finite d): +0 in all four channels,
 *     which the march reads as "no fog".
 * eye must be finite (VCT_EINVAL otherwise); pointer, alignment and size errors as
 * vct_sky_cones_device.  Needs no grid state.  Queued on the ctx stream. */
vct_status vct_fog_rays_device(vct_ctx* ctx, const vct_camera* cam, const float eye[3], const float* pos4,
                               uint32_t width, uint32_t height, float* ray4);

/* The march: fog4 = device [height][width][4] float (16-byte aligned) receives (F.rgb, T): the
 * light scattered toward the eye along the pixel's segment and the transmittance of the
 * segment.  The segment is clipped to the grid; a clipped-empty segment and a +0 ray record
 * give (0, 0, 0, 1).  steps: device counter (8-byte aligned), += the samples of this call, or
 * NULL.
 * Needs a current volume whose level equals fog->level (VCT_ESTATE otherwise; a stale or
 * missing volume too).  VCT_EINVAL: a fog that breaks the input rule, a non-finite eye (or
 * one whose voxel-unit position overflows), NULL or misaligned buffers, an empty frame.
 * Only density, level and step of `fog` are read by the march (albedo and ambient are in the
 * volume), so the density may change between frames without a rebuild.
 * Queued on the ctx stream; never waits for the device. */
vct_status vct_fog_march_device(vct_ctx* ctx, const vct_fog* fog, const float eye[3], const float* ray4,
                                uint32_t width, uint32_t height, float* fog4, unsigned long long* steps);

/* rgb = fmaf(rgb, T, F) per pixel on a composite's linear frame (any vct_composite_*'s
 * out_linear4), alpha untouched, background pixels included; with out_rgba8 the RGBA8 frame
 * of the result through the composite's own tone curve (alpha 255; a pixel whose alpha is 0, a
 * composite's background, keeps its clear colour outside the tone curve as the composite
 * presents it, and gets the fog over it: vct_spec.h).  Either output may be
 * NULL, not both; with linear4_inout NULL the frame is taken as +0, so out_rgba8 shows the
 * fog layer alone (rgb = F).  VCT_EINVAL, with nothing written: NULL fog4, both outputs NULL,
 * a misaligned buffer, an empty frame.  Needs no grid state.  Queued on the ctx stream. */
vct_status vct_fog_apply_device(vct_ctx* ctx, const float* fog4, uint32_t width, uint32_t height,
                                float* linear4_inout, uint32_t* out_rgba8);

#ifdef __cplusplus
}
#endif
#endif /* VCT_FOG_H */
