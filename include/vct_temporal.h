/*
 * vct_temporal.h — temporal accumulation: an additive extension of include/vct.h (which includes
 * this file; VCT_ABI_VERSION stays 1).
 *
 * Every other call computes a frame from nothing.  A grid that changes every frame (the dynamic
 * layer), a mixed-resolution trace and a coarse fog volume make the indirect term change from
 * frame to frame in ways a viewer sees as flicker.  The one call here carries per-pixel planes
 * from one frame to the next: it reprojects last frame's accumulated planes through last frame's
 * camera, keeps the taps whose surface agrees with this frame's pixel (the normal and plane
 * tests of the guided upsample, include/vct_mixed.h), and blends them with this frame's planes
 * as a running mean of bounded length.  include/vct_spec.h "temporal accumulation" has the exact
 * arithmetic; the call is a function of its inputs that tests/temporal_ref.py restates in
 * numpy, bit for bit.
 *
 * The call is stateless and image-space only: the history (accumulated planes, history lengths,
 * last frame's G-buffer and camera) lives in buffers the caller owns and swaps; the context
 * contributes only scratch of the stream for the per-wave stats words.  It is generic over any
 * [h][w][4] plane computed per G-buffer record (K4's diffuse plane, a sky plane, a shadow
 * plane), up to four at once, which then share one reprojection.
 *
 * Queued on the ctx stream; it never waits for the device (stats scratch that has to grow is
 * the exception, as K4's).  On a vct_create_multi context device 0 runs it, on device-0
 * pointers.  It needs no voxelization.  Implemented by the HIP library only, as the other
 * extension headers are.
 */
#ifndef VCT_TEMPORAL_H
#define VCT_TEMPORAL_H

#ifdef __cplusplus
extern "C" {
#endif

/* Default and limit of vct_temporal_params::max_len.  The default, normal_cos =
 * VCT_MIXED_NORMAL_COS and plane_eps = one voxel size are design choices, not measured optima:
 * DESIGN 10.9 reports the frame-to-frame stability and the response to a light change they give. */
#define VCT_TEMPORAL_DEFAULT_LEN 8u
#define VCT_TEMPORAL_MAX_LEN     1024u

/* normal_cos: finite, in [-1, 1].  plane_eps: finite, >= 0, sign bit clear (world units).
 * max_len: 1 .. VCT_TEMPORAL_MAX_LEN, the longest running mean (1: the call returns cur4).
 * Anything else is VCT_EINVAL with nothing written. */
typedef struct vct_temporal_params {
    float normal_cos;
    float plane_eps;
    uint32_t max_len;
} vct_temporal_params;

/* All pointers are device pointers; float planes are [height][width][4] and 16-byte aligned,
 * hist_len / out_len are [height][width] uint32, stats is [4] uint32 (4-byte aligned).
 * pos4 / nrm4: this frame's G-buffer (pos4.w != 0: a valid pixel, as K4 reads it).
 * motion4: NULL (nothing moved: a pixel's surface point was where it is), or per pixel xyz =
 * where this pixel's surface point was last frame, w = 0: it did not exist.
 * prev_cam: last frame's camera (its frame has this frame's width and height); NULL = no
 * history: every valid pixel resets, and prev_pos4 / prev_nrm4 / hist4 / hist_len are not read.
 * prev_pos4 / prev_nrm4: last frame's G-buffer.
 * n_planes: 1 .. 4 planes, entries [0, n_planes) of cur4 / hist4 / out4; the others are ignored.
 * cur4: this frame's planes.  hist4 / hist_len: last frame's out4 / out_len.
 * out4 / out_len: this frame's accumulated planes and history lengths (0 background, 1 reset,
 * k >= 2 a running mean over k frames).
 * stats: NULL, or {valid, reused, reset_offscreen, reset_rejected} counted over the frame's
 * pixels, valid = the sum of the other three; written, not accumulated.
 * Aliasing: out4[p] may equal cur4[p] (only the pixel's own value is read); out4[p] == hist4[q]
 * for any p, q, and out_len == hist_len, are VCT_EINVAL (a history is read at other pixels). */
typedef struct vct_temporal_args {
    uint32_t width, height;
    const float* pos4;
    const float* nrm4;
    const float* motion4;
    const vct_camera* prev_cam;
    const float* prev_pos4;
    const float* prev_nrm4;
    uint32_t n_planes;
    const float* cur4[4];
    const float* hist4[4];
    float* out4[4];
    const uint32_t* hist_len;
    uint32_t* out_len;
    uint32_t* stats;
} vct_temporal_args;

/* The header defaults for a context: normal_cos = VCT_MIXED_NORMAL_COS, plane_eps = one voxel
 * size (extent / n), max_len = VCT_TEMPORAL_DEFAULT_LEN. */
vct_status vct_temporal_default_params(const vct_ctx* ctx, vct_temporal_params* out);

/* out4 / out_len from cur4 and the reprojected hist4 / hist_len (vct_spec.h "temporal
 * accumulation"): background pixels +0 and length 0; a pixel whose previous position leaves
 * last frame's view, whose taps all fail the tests, or whose blended history is not finite
 * resets to cur4 bit for bit with length 1; the others get H + (cur - H) / k.
 * VCT_EINVAL, nothing written: params outside their rule; width or height 0 (or above 65536, or
 * more than 2^31 - 1 pixels); n_planes 0 or > 4; a NULL or misaligned pos4, nrm4, cur4[p],
 * out4[p] or out_len, a misaligned motion4 or stats; a prev_cam whose tan(zoom / 2) is not
 * finite and > 0 or whose vectors or position are not finite; with prev_cam, a NULL or
 * misaligned prev_pos4, prev_nrm4, hist4[p] or hist_len; the aliasing above. */
vct_status vct_temporal_accumulate_device(vct_ctx* ctx, const vct_temporal_args* args,
                                          const vct_temporal_params* params);

#ifdef __cplusplus
}
#endif
#endif /* VCT_TEMPORAL_H */
