/*
 * vct_mixed.h — mixed-resolution trace: an additive extension of include/vct.h (which includes
 * this file; VCT_ABI_VERSION stays 1).
 *
 * K4's diffuse cones compute wide-aperture irradiance, which is low in frequency everywhere but
 * at geometric edges.  The functions here trace them on a frame 2 or 4 times smaller per axis,
 * upsample the result under the guidance of the full-resolution G-buffer, trace exactly the
 * pixels no low-resolution sample fits ("holes"), and keep full resolution for the specular
 * cone alone.  include/vct_spec.h "mixed-resolution trace" has the exact arithmetic; every step
 * is a function of its inputs that tests/mixed_ref.py restates in numpy, bit for bit.
 *
 *   vct_trace_cones_device     K4 with a cone selection: the diffuse set, the specular cone, or both
 *   vct_mixed_pick_device      full G-buffer -> low G-buffer (the nearest valid pixel of each block)
 *   vct_mixed_upsample_device  low plane -> full plane, plus the packed list of holes
 *   vct_mixed_scatter_device   traced hole values -> their pixels
 *   vct_trace_mixed_device     the frame call: the five steps above and the specular launch
 *
 * The upsample is generic over any [h][w][4] plane computed per G-buffer record: K4's diffuse
 * plane, the sky plane of vct_sky_cones_device, a shadow plane.
 *
 * All of them are queued on the ctx stream and never wait for the device (scratch that has to
 * grow is K4's exception, as in vct_trace_device); their scratch belongs to the stream, as
 * K4's does.  On a vct_create_multi context device 0 runs them, on device-0 pointers.  They
 * need a voxelization and built mips (VCT_ESTATE otherwise).  Implemented by the HIP library
 * only, as the other extension headers are.
 */
#ifndef VCT_MIXED_H
#define VCT_MIXED_H

#ifdef __cplusplus
extern "C" {
#endif

#define VCT_CONES_DIFFUSE   1u
#define VCT_CONES_SPECULAR  2u

/* Default of vct_mixed_params::normal_cos (vct_mixed_default_params).  It and the default
 * plane_eps (`factor` voxel sizes) are design choices, not measured optima: DESIGN 10.7 reports
 * the hole shares and the error they produce. */
#define VCT_MIXED_NORMAL_COS 0.9f
/* Width in pixels of the packed hole G-buffer (one K4 wave row of 8x8 blocks per 64 holes). */
#define VCT_MIXED_HOLE_WIDTH 64u
#define VCT_MIXED_NO_SOURCE  0xffffffffu   /* lo_src of a block without a valid pixel */

/* normal_cos: finite, in [-1, 1].  plane_eps: finite, >= 0, sign bit clear (world units).
 * max_holes: capacity of the hole list, >= 1; 0 means ceil(width * height / 8).
 * factor: 2 or 4; read by vct_trace_mixed_device only (the other calls take it as an argument).
 * Anything else is VCT_EINVAL with nothing written. */
typedef struct vct_mixed_params {
    float normal_cos;
    float plane_eps;
    uint32_t max_holes;
    uint32_t factor;
} vct_mixed_params;

/* The hole list of one upsample.  With M = max_holes and R = ceil(M / 64):
 * pos4 / nrm4 / alb4: device [R][64][4] float (16-byte aligned), the packed hole G-buffer, a
 * frame K4 (or any per-pixel march) traces as it stands: entry k holds hole k's three records,
 * every entry from min(count, M) on is +0 (a background pixel).
 * px: device [M] uint32, the pixel index y * width + x of hole k.
 * count: device [1] uint32, the number of holes of the frame (it may exceed M: the holes from M
 * on are overflows and carry the fallback value).
 * stats: NULL, or device [4] uint32 = {representatives, interpolated, holes, overflowed},
 * counted over valid pixels; written, not accumulated.
 * max_holes: M; it must equal the params' capacity (after its 0 -> default rule). */
typedef struct vct_mixed_holes {
    float* pos4;
    float* nrm4;
    float* alb4;
    uint32_t* px;
    uint32_t* count;
    uint32_t* stats;
    uint32_t max_holes;
} vct_mixed_holes;

/* The header defaults for a context and factor: normal_cos = VCT_MIXED_NORMAL_COS, plane_eps =
 * factor voxel sizes (factor * extent / n), max_holes = 0. */
vct_status vct_mixed_default_params(const vct_ctx* ctx, uint32_t factor, vct_mixed_params* out);

/* vct_trace_device restricted to the cones of `cones` (VCT_CONES_DIFFUSE, VCT_CONES_SPECULAR,
 * or both = vct_trace_device itself).  The selected plane equals the same plane of
 * vct_trace_device on the same arguments bit for bit, in every public variant; steps_px,
 * cone_steps and texel_fetches count the selected cones only.  The unselected plane pointer may
 * be NULL and is not written.  Selecting cones the context lacks (n_diffuse = 0, specular = 0)
 * writes +0 to the selected plane (and 0 steps).  The tuner (vct_trace_form) keeps one workload
 * per cone set.  VCT_EINVAL: cones 0 or > 3, and what vct_trace_device refuses. */
vct_status vct_trace_cones_device(vct_ctx* ctx, const vct_trace_args* args, uint32_t cones);

/* Low frame: wl = ceil(width / factor) by hl = ceil(height / factor).  Low pixel (X, Y) takes,
 * bit for bit, the three records of the valid pixel (pos.w != 0) of its factor x factor block
 * nearest to `eye` (squared distance in float32; a NaN distance counts as +Inf; ties go to the
 * lower pixel index), and lo_src[Y][X] = that pixel's index y * width + x.  A block without a
 * valid pixel gets +0 records and VCT_MIXED_NO_SOURCE.  lo_*4: device [hl][wl][4] float;
 * lo_src: device [hl][wl] uint32. */
vct_status vct_mixed_pick_device(vct_ctx* ctx, const float* pos4, const float* nrm4, const float* alb4,
                                 uint32_t width, uint32_t height, const float eye[3], uint32_t factor,
                                 float* lo_pos4, float* lo_nrm4, float* lo_alb4, uint32_t* lo_src);

/* plane4[h][w][4] from lo_plane4[hl][wl][4] (vct_spec.h "mixed-resolution trace"): background
 * pixels +0, representatives their low pixel's value, the others the bilinear blend of the taps
 * whose normal and plane agree with the pixel's; a pixel without such a tap is a hole: listed
 * in `holes` in row-major order, its plane value left untouched for the scatter (an overflow
 * gets the blend of every tap instead).  alb4 is only copied into the hole G-buffer. */
vct_status vct_mixed_upsample_device(vct_ctx* ctx, const float* pos4, const float* nrm4, const float* alb4,
                                     uint32_t width, uint32_t height, uint32_t factor, const float* lo_pos4,
                                     const float* lo_nrm4, const uint32_t* lo_src, const float* lo_plane4,
                                     const vct_mixed_params* params, float* plane4, const vct_mixed_holes* holes);

/* plane4[holes->px[k]] = hole_plane4[k] for k < min(*holes->count, holes->max_holes); the count
 * is read on the device.  hole_plane4: device [R][64][4], what was traced over the hole
 * G-buffer.  holes->px must hold pixel indices of plane4's frame (an upsample's list does). */
vct_status vct_mixed_scatter_device(vct_ctx* ctx, const float* hole_plane4, const vct_mixed_holes* holes,
                                    float* plane4);

/* The frame: pick -> K4 diffuse cones on the low frame -> upsample into args->diffuse4 -> K4
 * diffuse cones on the hole frame -> scatter -> K4 specular cone at full resolution into
 * args->spec4.  cone_steps and texel_fetches accumulate over the three K4 launches.  steps_px
 * must be NULL and tile_world / tile_compact 0 (VCT_EINVAL otherwise, nothing written); the
 * variant goes to every K4 launch. */
vct_status vct_trace_mixed_device(vct_ctx* ctx, const vct_trace_args* args, const vct_mixed_params* params);

#ifdef __cplusplus
}
#endif
#endif /* VCT_MIXED_H */
