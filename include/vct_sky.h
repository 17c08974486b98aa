/*
 * vct_sky.h — sky light: an additive extension of include/vct.h (which includes this file;
 * VCT_ABI_VERSION stays 1).
 *
 * A cone that leaves the grid returns +0 (include/vct_spec.h A.6), so without this extension
 * a surface the sun does not reach is lit only by what bounces off sunlit voxels.  The two
 * functions here add a sky: for every receiver, the context's diffuse cone set is marched
 * through the alpha of the radiance pyramid (the march of "shadow cones", unlimited: K4's own
 * diffuse cones reduced to their alpha channel), and each cone sees the sky colour of its
 * direction through the transmittance T it ends with.  include/vct_spec.h "sky light" has the
 * exact arithmetic.  vct_sky_cones_device does it per pixel and can add the result to K4's
 * diffuse plane, so that every composite shows the sky through its albedo x diffuse term;
 * vct_inject_sky does it per voxel, so that sky light bounces and shows up in reflections.
 *
 * They live in their own header for the reason vct_bounce.h, vct_lights.h, vct_shadow.h and
 * vct_emission.h do: vct.h's text is the list of symbols every implementation of the boundary
 * exports, and these are implemented by the HIP library only.
 *
 * Call order:  vct_voxelize* -> vct_inject_* [-> vct_inject_emission] -> vct_build_mips
 *              [-> vct_inject_sky] [-> vct_inject_bounces] -> vct_trace*
 *              [-> vct_sky_cones_device] -> vct_composite_*
 *
 * The vct_sky record is read during the call; it is not kept in the context.
 */
#ifndef VCT_SKY_H
#define VCT_SKY_H

#ifdef __cplusplus
extern "C" {
#endif

/* The sky: a colour for straight up (zenith), for the horizon and for straight down (ground),
 * blended by the cosine between a direction and `up`.  Input rule: the float32 length of `up`
 * must be finite and > 0 (the K2 direction rule; `up` is normalised as vct_inject_directional
 * normalises its direction); every colour component must be finite, have a clear sign bit
 * (-0.0f is refused) and be <= VCT_COLOR_LIMIT.  Anything else is VCT_EINVAL, with nothing
 * written and no state changed. */
typedef struct vct_sky {
    float up[3];
    float zenith[3];
    float horizon[3];
    float ground[3];
} vct_sky;

/* Per pixel: sky4 = device [height][width][4] float (16-byte aligned) receives (Sk.rgb, vis),
 * vis = the cone-weighted transmittance toward the sky; +0 in all four channels for a
 * background pixel (pos.w == 0) and when the context has n_diffuse = 0.
 * diffuse4_inout: NULL, or K4's diffuse plane of the same frame (16-byte aligned): at every
 * valid pixel diffuse.rgb = diffuse.rgb + Sk.rgb (one add per channel), alpha untouched.
 * cone_steps: device counter (8-byte aligned), += the cone steps of this call, or NULL; a sky
 * call takes exactly the steps of K4's diffuse cones on the same frame.
 * The step table of the diffuse aperture is one of the context's tables (vct_shadow.h): a sky
 * call and a shadow call of one context run in the order they were made whatever streams they
 * are queued on.
 * Needs a voxelization and built mips (VCT_ESTATE otherwise).  VCT_EINVAL, with nothing
 * written: a sky that breaks the input rule, NULL sky, NULL or misaligned sky4 / pos4 / nrm4 /
 * diffuse4_inout / cone_steps, width or height 0.  Queued on the ctx stream; never waits for
 * the device.  On a vct_create_multi context device 0 runs it, on device-0 pointers. */
vct_status vct_sky_cones_device(vct_ctx* ctx, const float* pos4, const float* nrm4,
                                uint32_t width, uint32_t height, const vct_sky* sky,
                                float* sky4, float* diffuse4_inout, unsigned long long* cone_steps);

/* Per voxel: at every bounce source (vct_bounce.h: an occupied voxel with a nonzero normal)
 * L.rgb = L.rgb + A.rgb * Sk.rgb on level 0 (one multiply, one add per channel; alpha
 * untouched), with Sk from the same march over the source's G-buffer record, then the mips
 * are rebuilt (vct_build_mips: on a multi-device context device 0 does the add, and the
 * result travels with the build's level-0 copy).  The nonzero pattern of level 0 and the
 * alpha of every level are unchanged.
 * Needs a voxelization, a level 0 and built mips; allowed once per level 0, and only before
 * vct_inject_bounces on that level 0 (the bounce's L0 must already hold the sky);
 * VCT_ESTATE otherwise.  Every new level 0 (inject, upload, load) re-arms it.  Waits for the
 * ctx stream once when the source list of a new voxelization has to be built, as
 * vct_inject_bounces does. */
vct_status vct_inject_sky(vct_ctx* ctx, const vct_sky* sky);

#ifdef __cplusplus
}
#endif
#endif /* VCT_SKY_H */
