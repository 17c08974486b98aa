/*
 * vct_sky_view.h — the sky in view: an additive extension of include/vct.h (which includes
 * this file; VCT_ABI_VERSION stays 1).
 *
 * vct_sky.h brings the sky into the diffuse term and into level 0.  Two places where a viewer
 * looks straight at the sky are left: K4's specular cone returns +0 once it leaves the grid
 * (include/vct_spec.h A.6), so a glossy floor under an open roof reflects black, and every
 * composite writes the clear colour behind the geometry.  The two functions here fill them:
 * vct_sky_specular_device marches the specular cone of every pixel through the alpha of the
 * pyramid (K4's own specular cone reduced to its alpha channel) and shows the sky colour of
 * the reflected direction through the transmittance it ends with; vct_sky_background_device
 * writes the sky colour of the primary ray at every background pixel of a composited frame.
 * include/vct_spec.h "sky in view" has the exact arithmetic.
 *
 * They live in their own header for the reason vct_sky.h does: vct.h's text is the list of
 * symbols every implementation of the boundary exports, and these are implemented by the HIP
 * library only.
 *
 * Call order:  ... vct_trace* [-> vct_sky_cones_device] [-> vct_sky_specular_device]
 *              -> vct_composite_* [-> vct_sky_background_device] [-> vct_fog_apply_device]
 *
 * The vct_sky record (vct_sky.h, with its input rule) is read during the call.
 */
#ifndef VCT_SKY_VIEW_H
#define VCT_SKY_VIEW_H

#ifdef __cplusplus
extern "C" {
#endif

/* Per pixel: skyspec4 = device [height][width][4] float (16-byte aligned) receives (S.rgb, T):
 * T = the transmittance of the pixel's specular cone (K4's: reflected direction, aperture
 * clamp(roughness = alb.w)), S = T * Sky(r); +0 in all four channels for a background pixel
 * (pos.w == 0) and when the context has specular = 0.
 * spec4_inout: NULL, or K4's specular plane of the same frame (16-byte aligned): at every
 * valid pixel spec.rgb = spec.rgb + S.rgb (one add per channel), alpha untouched.
 * cone_steps: device counter (8-byte aligned), += the cone steps of this call, or NULL; a call
 * takes exactly the steps of K4's specular cones on the same frame.
 * The aperture is per pixel; each lane derives its own steps, so the context's step tables
 * (vct_shadow.h) are not involved and the call orders with nothing but its stream.
 * Needs a voxelization and built mips (VCT_ESTATE otherwise).  VCT_EINVAL, with nothing
 * written: a sky that breaks vct_sky's input rule, NULL sky, NULL eye, NULL or misaligned
 * pos4 / nrm4 / alb4 / skyspec4, misaligned spec4_inout / cone_steps, width or height 0.
 * Queued on the ctx stream; never waits for the device.  On a vct_create_multi context device
 * 0 runs it, on device-0 pointers. */
vct_status vct_sky_specular_device(vct_ctx* ctx, const float* pos4, const float* nrm4, const float* alb4,
                                   uint32_t width, uint32_t height, const float eye[3], const vct_sky* sky,
                                   float* skyspec4, float* spec4_inout, unsigned long long* cone_steps);

/* Per background pixel (pos.w == 0; -0.0f is background) of a composited frame:
 * linear4_inout[px] = (Sky(d).rgb, 1.0f) and rgba8_inout[px] = the tone curve of Sky(d) with
 * alpha 255, packed as the composites pack it; d = the primary ray of the pixel through cam
 * (the G-buffer caster's).  Alpha 1 makes vct_fog_apply_device take the pixel through the
 * tone curve like a surface, not as a clear-colour pixel.  Valid pixels are not touched in
 * either buffer.  linear4_inout (16-byte aligned) or rgba8_inout (4-byte aligned) may be NULL,
 * not both.  Needs no grid state.  VCT_EINVAL, with nothing written: a sky that breaks the
 * input rule, NULL cam / pos4 / sky, both outputs NULL, a misaligned buffer, width or height
 * 0.  Queued on the ctx stream; never waits for the device. */
vct_status vct_sky_background_device(vct_ctx* ctx, const vct_camera* cam, const float* pos4,
                                     uint32_t width, uint32_t height, const vct_sky* sky,
                                     float* linear4_inout, uint32_t* rgba8_inout);

#ifdef __cplusplus
}
#endif
#endif /* VCT_SKY_VIEW_H */
