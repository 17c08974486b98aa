/*
 * vct_lights.h — point and spot lights: an additive extension of include/vct.h (which
 * includes this file; VCT_ABI_VERSION stays 1).
 *
 * vct_inject_directional lights the grid with one directional light and
 * vct_composite_device takes one dir_to_light.  The two functions here take a list of
 * lights instead -- directional, point and spot, in any mix -- and sum their direct terms
 * in list order (include/vct_spec.h "local lights" has the exact arithmetic: a smooth
 * window to zero at `range` over an inverse-square falloff, a smoothstep-squared spot
 * cone, and the K2 shadow walk ended where it reaches the light).
 *
 * They live in their own header for the reason vct_bounce.h does: vct.h's text is the
 * list of symbols that every implementation of the boundary exports (the CPU oracle
 * backend included), and these are implemented by the HIP library only.
 *
 * Call order:  vct_voxelize*  ->  vct_inject_lights  ->  vct_build_mips
 *              [-> vct_inject_bounces]  ->  vct_trace*  ->  vct_composite_lights_device
 *
 * The list is read during the call; it is not kept in the context.  The order of the
 * list is part of the result: float addition is not associative, so two orders of the
 * same lights may differ in the last bit of a voxel that several of them reach.
 */
#ifndef VCT_LIGHTS_H
#define VCT_LIGHTS_H

#ifdef __cplusplus
extern "C" {
#endif

#define VCT_LIGHT_DIRECTIONAL 0u
#define VCT_LIGHT_POINT       1u
#define VCT_LIGHT_SPOT        2u
#define VCT_MAX_LIGHTS        64u

typedef struct vct_light {      /* 60 bytes, host memory */
    uint32_t type;
    float position[3];   /* world; point, spot                                         */
    float direction[3];  /* directional: toward the light (as vct_inject_directional);
                            spot: the axis the spot shines along (away from the light) */
    float color[3];      /* finite, >= 0 (not -0.0f), <= VCT_COLOR_LIMIT (vct_spec.h)  */
    float range;         /* world units, > 0; point, spot: no light at distance >= range */
    float cos_inner;     /* spot: full intensity inside, 1 >= cos_inner > cos_outer >= 0 */
    float cos_outer;     /* spot: no light outside                                     */
    uint32_t reserved[2];/* 0                                                          */
} vct_light;

/* K2 for a list of lights: replaces the level-0 radiance, exactly as
 * vct_inject_directional does (same state effects; level 0 stays nonzero exactly at the
 * occupied voxels, alpha 1, so the next vct_build_mips may be a relight build).
 * n_lights = 0 is valid: a dark grid, (0,0,0,1) at every occupied voxel.
 * Fields a light's type does not use (a directional light's position, range and cosines,
 * a point light's direction and cosines) are ignored but must be finite.
 * VCT_ESTATE before a voxelization.  VCT_EINVAL, with nothing changed: NULL lights with
 * n_lights > 0, n_lights > VCT_MAX_LIGHTS, an unknown type, a non-finite field, a negative
 * colour or one above VCT_COLOR_LIMIT, a direction whose float32 length is not finite and > 0
 * where one is used (vct_spec.h "K2 input rule"), range <= 0 (point, spot), cosines that break
 * 1 >= cos_inner > cos_outer >= 0 (spot), nonzero reserved words.
 * Queued on the ctx stream; never waits for the device.  On a vct_create_multi context
 * device 0 injects; the result reaches the other devices with vct_build_mips. */
vct_status vct_inject_lights(vct_ctx* ctx, const vct_light* lights, uint32_t n_lights);

/* vct_composite_device with the direct term summed over `lights` (n_lights = 0: no direct
 * term).  Every other precondition and output is vct_composite_device's, the start of a
 * pixel's shadow walks included (vct_spec.h "shadow-walk receiver rule": V = 1 for a pixel
 * whose cone origin is NaN or outside the grid); the lights are validated as by
 * vct_inject_lights. */
vct_status vct_composite_lights_device(vct_ctx* ctx, const float* pos4, const float* nrm4, const float* alb4,
                                       const float* diffuse4, const float* spec4, uint32_t width, uint32_t height,
                                       const vct_light* lights, uint32_t n_lights,
                                       float* out_linear4, uint32_t* out_rgba8);

#ifdef __cplusplus
}
#endif
#endif /* VCT_LIGHTS_H */
