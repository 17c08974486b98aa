/*
 * vct_motion.h — object motion: an additive extension of include/vct.h (which includes this
 * file after vct_objects.h and vct_temporal.h; VCT_ABI_VERSION stays 1).
 *
 * vct_temporal_accumulate_device takes a motion4 plane: per pixel, where the pixel's surface
 * point was last frame, w = 0 meaning nowhere.  The two calls here produce that plane for the
 * object set of include/vct_objects.h: the set remembers the last pose given to every object,
 * the shaded G-buffer pass (vct_gbuffer_shaded_device / vct_gbuffer_cutout_device) names the
 * triangle and the barycentrics of every pixel, and the set keeps its object-space vertices on
 * the device; a pixel on a moved object is therefore the same point of the same triangle under
 * last frame's matrix.  include/vct_spec.h "object motion" has the exact arithmetic, which
 * tests/motion_ref.py restates in numpy, bit for bit.
 *
 * Call order, per frame:
 *     vct_objects_update*            (the objects that moved)
 *     vct_gbuffer_shaded_device      (pos4, nrm4, tri_id, bary2)
 *     vct_objects_motion_device      (motion4, prev_nrm4 from last frame's snapshot)
 *     vct_inject_* / vct_build_mips / vct_trace*
 *     vct_temporal_accumulate_device (motion4 = motion4; nrm4 = prev_nrm4: see below)
 *     vct_objects_poses_device       (the snapshot for the next frame)
 *
 * The normal plane
 *   The accumulate's tap tests compare this frame's normal with last frame's G-buffer.  A
 *   rotating object fails the normal test although its history is valid.  prev_nrm4 is the
 *   pixel's normal under last frame's pose (nrm4 itself on every pixel that did not move):
 *   given to the accumulate as its nrm4, both tap tests are those of a surface that stood
 *   still.  The history a host keeps for the next frame stores the real nrm4.
 *
 * vct_objects_motion_device is stateless: last frame's poses belong to the caller, as last
 * frame's planes belong to the caller of vct_temporal.  Both calls are queued on the ctx stream
 * and never wait for the device (stats scratch that has to grow is the exception, as in
 * vct_temporal.h).  On a vct_create_multi context device 0 runs them, on device-0 pointers.
 * Implemented by the HIP library only, as the other extension headers are.
 */
#ifndef VCT_MOTION_H
#define VCT_MOTION_H

#ifdef __cplusplus
extern "C" {
#endif

/* Queues a copy of the set's n_objects current poses into out (device, 16-byte aligned): the
 * last pose given to each object, exactly as given; all zero (so visible == 0) for an object
 * that never had one.  capacity < n_objects, NULL or misaligned: VCT_EINVAL.  No set:
 * VCT_ESTATE.  Never waits. */
vct_status vct_objects_poses_device(vct_ctx* ctx, vct_object_pose* out, uint32_t capacity);

/* All pointers are device pointers.  float4 planes and prev_poses are 16-byte aligned, bary2
 * 8-byte, tri_id and stats 4-byte. */
typedef struct vct_motion_args {
    uint32_t width, height;
    const float*    pos4;      /* [h][w][4], this frame's G-buffer (w != 0: valid) */
    const float*    nrm4;      /* [h][w][4]; NULL iff prev_nrm4 is NULL */
    const uint32_t* tri_id;    /* [h][w], as vct_gbuffer_shaded_device / _cutout_device write it */
    const float*    bary2;     /* [h][w][2] */
    const vct_object_pose* prev_poses;  /* device, n_prev records: the set's poses at last frame's end */
    uint32_t n_prev;           /* must equal the set's n_objects */
    float*    motion4;         /* out [h][w][4]: vct_temporal_args::motion4 */
    float*    prev_nrm4;       /* out, NULL ok: the pixel's normal under last frame's pose */
    uint32_t* stats;           /* NULL ok: {valid, static_or_unmoved, moved, appeared} */
} vct_motion_args;

/* motion4 / prev_nrm4 by the rule of vct_spec.h "object motion": a background pixel +0; a pixel
 * on a static triangle, or on an object whose matrix is the snapshot's in every bit, (pos4.xyz, 1)
 * and nrm4; a pixel on an object that moved, the same point of its triangle under the
 * snapshot's matrix, and that triangle's normal under it; a pixel whose object was hidden in
 * the snapshot, whose id names no triangle, or whose previous point is not finite, motion4 = 0
 * (the accumulate resets it) and nrm4.  stats is written, not accumulated: valid = the sum of
 * the other three.
 * VCT_EINVAL, nothing written: a NULL pos4, tri_id, bary2, prev_poses or motion4; a misaligned
 * buffer; width or height 0 (or above 65536, or more than 2^31 - 1 pixels); exactly one of nrm4
 * and prev_nrm4; n_prev != the set's n_objects.  VCT_ESTATE, nothing written: no set is
 * defined.  Pixel contents, ids, barycentrics and matrix contents are data, never a status. */
vct_status vct_objects_motion_device(vct_ctx* ctx, const vct_motion_args* args);

#ifdef __cplusplus
}
#endif
#endif /* VCT_MOTION_H */
