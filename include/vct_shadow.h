/*
 * vct_shadow.h — cone-traced soft shadows: an additive extension of include/vct.h (which
 * includes this file; VCT_ABI_VERSION stays 1).
 *
 * vct_composite_device and vct_composite_lights_device shade their direct term with the K2
 * voxel walk: a binary test against the level-0 occupancy bits, so every shadow edge is a
 * staircase one voxel wide and a light's size has no effect.  The two functions here split
 * that term: vct_shadow_cones_device writes a visibility V in [0, 1] for every (light,
 * pixel), marching one cone per pair toward the light through the alpha of the radiance
 * pyramid (include/vct_spec.h "shadow cones" has the exact arithmetic: K4's march reduced
 * to its alpha channel, ended where it reaches the light), and
 * vct_composite_shadowed_device is vct_composite_lights_device with V read from that plane.
 * A light whose tan_half is 0 keeps the hard walk, so an all-zero tan_half reproduces
 * vct_composite_lights_device bit for bit.
 *
 * They live in their own header for the reason vct_bounce.h and vct_lights.h do: vct.h's
 * text is the list of symbols every implementation of the boundary exports, and these are
 * implemented by the HIP library only.
 *
 * Call order:  ... -> vct_build_mips [-> vct_inject_bounces] -> vct_trace*
 *              -> vct_shadow_cones_device -> vct_composite_shadowed_device
 *
 * The light list and tan_half are read during the call; neither is kept in the context.
 */
#ifndef VCT_SHADOW_H
#define VCT_SHADOW_H

#ifdef __cplusplus
extern "C" {
#endif

/* V for every (light, pixel): vis = device [n_lights][height][width] float (4-byte aligned).
 * tan_half = host [n_lights]; tan_half[j] == 0: light j keeps the hard voxel walk (V in {0,1});
 * > 0: a shadow cone of that half-angle tangent, clamped to [VCT_SPEC_TAU_MIN, VCT_SPEC_TAU_MAX].
 * vis[j][y][x] is +0 for a background pixel and for a light the pixel skips (facing away,
 * out of range, outside the spot cone).
 * A pixel whose cone origin has a NaN component, or lies far outside the grid, is legal: a hard
 * light gives it V = 1 without a walk (vct_spec.h "shadow-walk receiver rule"), a soft light
 * V = 1 with no cone step, so the two agree.
 * cone_steps: device counter (8-byte aligned), += the cone steps of this call, or NULL.
 * The context keeps one small step table per distinct clamped aperture it has met, built on
 * the device by the first call that uses it.  The tables belong to the context, not to a
 * stream: a call queued on another stream than the context's previous call of this function
 * first makes its stream wait, on the device, for that call's end, so calls of one context
 * run in the order they were made whatever streams they are queued on.
 * Needs a voxelization and built mips (VCT_ESTATE otherwise).  VCT_EINVAL, with nothing
 * written: whatever vct_inject_lights rejects in a light, n_lights > VCT_MAX_LIGHTS, NULL
 * tan_half with n_lights > 0, a tan_half entry that is negative, NaN or infinite, NULL or
 * misaligned vis / pos4 / nrm4 (16 bytes for the float4 planes), width or height 0.
 * n_lights = 0 is a no-op.  Queued on the ctx stream; never waits for the device.  On a
 * vct_create_multi context device 0 runs it, on device-0 pointers. */
vct_status vct_shadow_cones_device(vct_ctx* ctx, const float* pos4, const float* nrm4,
                                   uint32_t width, uint32_t height,
                                   const vct_light* lights, uint32_t n_lights, const float* tan_half,
                                   float* vis, unsigned long long* cone_steps);

/* vct_composite_lights_device with V read from vis[j][pixel] instead of walked: every other
 * precondition and output is that function's.  vis: NULL or misaligned with n_lights > 0 is
 * VCT_EINVAL.  n_lights = 0: no direct term (vis is not read). */
vct_status vct_composite_shadowed_device(vct_ctx* ctx, const float* pos4, const float* nrm4, const float* alb4,
                                         const float* diffuse4, const float* spec4,
                                         uint32_t width, uint32_t height,
                                         const vct_light* lights, uint32_t n_lights, const float* vis,
                                         float* out_linear4, uint32_t* out_rgba8);

#ifdef __cplusplus
}
#endif
#endif /* VCT_SHADOW_H */
