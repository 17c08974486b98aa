/*
 * vct_voxview.h — the voxel view and ray picking: an additive extension of include/vct.h
 * (which includes this file; VCT_ABI_VERSION stays 1).
 *
 * Every stage of the path can be compared with the oracle, and none of it could be looked at
 * without copying whole volumes to the host.  The two calls here walk rays cell by cell through
 * one level of the radiance pyramid, or through K1's occupancy bits, and report the first solid
 * cell each ray meets:
 *
 *   vct_voxel_pick_device   a list of arbitrary rays -> one hit record per ray: which cell, through
 *                           which face, how far, after how many cells.  Mouse picking in an
 *                           editor, line-of-sight tests, anything that is not voxelized.
 *   vct_voxel_view_device   the same walk over the primary rays of a camera, generated in
 *                           registers, with the hit cell coloured by what the level holds: a frame
 *                           that shows what K1 voxelized, what K2 / a light list / a bounce / the
 *                           sky put into level 0, what the mips look like from a given side, and
 *                           where the dynamic layer's voxels are.
 *
 * Both run the one device function, so the view's hit records equal the pick's on the rays
 * (org = cam->position, dir = the caster's pixel ray) in every bit.  The walk is exact: the cells
 * a ray tests are the cells it passes through in the float32 arithmetic of include/vct_spec.h
 * "voxel view", nothing is filtered.  (The fog march is the sampled path through the pyramid.)
 *
 * Like vct_query.h, the functions are implemented by the HIP library only.
 *
 * Call order:  vct_voxelize* -> [vct_inject_* | vct_upload_level0 -> vct_build_mips]
 *              -> vct_voxel_pick_device | vct_voxel_view_device
 */
#ifndef VCT_VOXVIEW_H
#define VCT_VOXVIEW_H

#ifdef __cplusplus
extern "C" {
#endif

/* what makes a cell solid for a pick */
#define VCT_VOXPICK_OCCUPANCY 0   /* K1's occupancy bit; level 0 only; needs a voxelization       */
#define VCT_VOXPICK_ALPHA     1   /* alpha > 0 in any face of the cell's level-l texel (a NaN is
                                     not solid); level 0 needs an injected or uploaded level 0,
                                     a level >= 1 built mips                                      */

/* what the view shows; the solid source each mode implies is in the right column */
#define VCT_VOXVIEW_RADIANCE  0   /* rgb of the level-l texel (A.5's face blend above level 0): ALPHA      */
#define VCT_VOXVIEW_ALPHA     1   /* the same combination's alpha in all three channels:        ALPHA      */
#define VCT_VOXVIEW_ALBEDO    2   /* albedo_occ.rgb; level 0 only:                              OCCUPANCY  */
#define VCT_VOXVIEW_NORMAL    3   /* fmaf(0.5f, n_c, 0.5f); level 0 only:                       OCCUPANCY  */

/* a hit record: uint32 (cell, face, steps, float bits of t) */
#define VCT_VOXHIT_FACE_INSIDE 6u          /* the origin lies in a solid cell                     */
#define VCT_VOXHIT_FACE_MISS   7u
#define VCT_VOXHIT_CELL_MISS   0xFFFFFFFFu

typedef struct vct_voxel_pick_args {
    const float* org4;          /* device [count][4], 16-byte aligned: origin, world units (.w unused) */
    const float* dir4;          /* device [count][4], 16-byte aligned: direction (any length), and
                                   .w = t_lim in level-0 voxel units; +Inf or NaN: no limit      */
    uint32_t count;
    uint32_t level;             /* 0 .. L                                                        */
    uint32_t solid;             /* VCT_VOXPICK_*                                                 */
    uint32_t* hit4;             /* device [count][4] uint32, 16-byte aligned:
                                   cell  = x + n_l (y + n_l z) at the level,
                                   face  = the entry face 0..5 (-x, +x, -y, +y, -z, +z), or
                                           VCT_VOXHIT_FACE_INSIDE,
                                   steps = cells this ray tested,
                                   t     = float bits of the entry distance along the normalised
                                           direction, level-0 voxel units.
                                   A miss is (VCT_VOXHIT_CELL_MISS, VCT_VOXHIT_FACE_MISS, steps,
                                   bits of +Inf).                                                */
    unsigned long long* cells;  /* device counter (8-byte aligned), += the cells tested, or NULL */
} vct_voxel_pick_args;

/* Walks every ray of the list (include/vct_spec.h "voxel view").  One ray per lane, in list
 * order; no ray depends on another, so a permuted list gives the permuted records.  Rays of a
 * wave that run through different parts of the grid pay for each other's loads: order the list
 * spatially where it matters -- the call does not sort.
 * Ray contents are device data and never a status: a zero, NaN or infinite direction or origin
 * is a miss with 0 steps.
 * VCT_EINVAL, with nothing written: NULL args, org4, dir4 or hit4; org4 / dir4 / hit4 not
 * 16-byte aligned, cells not 8-byte aligned; level > L; a `solid` outside VCT_VOXPICK_*;
 * VCT_VOXPICK_OCCUPANCY with level != 0.  VCT_ESTATE when the state named above is missing.
 * count == 0 is VCT_OK and launches nothing.  Queued on the ctx stream; never waits for the
 * device.  On a vct_create_multi context device 0 runs it, on device-0 pointers. */
vct_status vct_voxel_pick_device(vct_ctx* ctx, const vct_voxel_pick_args* args);

typedef struct vct_voxel_view_args {
    uint32_t width, height;
    uint32_t level;             /* 0 .. L; 0 for ALBEDO and NORMAL                               */
    uint32_t mode;              /* VCT_VOXVIEW_*                                                 */
    uint32_t shade;             /* 1: the colour is multiplied by VCT_VOXVIEW_SHADE_X / _Y / _Z
                                   (include/vct_spec.h) by the entry face's axis, so cubes read
                                   as cubes (1.0 for VCT_VOXHIT_FACE_INSIDE); 0: by nothing      */
    float* linear4;             /* device [h][w][4], 16-byte aligned, or NULL: (rgb, 1.0f) on a
                                   hit, +0 in all four on a miss -- the composites' alpha
                                   convention, so vct_fog_apply_device takes the frame           */
    uint32_t* rgba8;            /* device [h][w] (4-byte aligned) or NULL: alpha 255 on a hit,
                                   RADIANCE through the composites' present step, the other
                                   modes rounded to 8 bits without the tone curve; 0 on a miss   */
    uint32_t* hit4;             /* device [h][w][4] or NULL: the records of the pick             */
    unsigned long long* cells;  /* as the pick's, or NULL                                        */
} vct_voxel_view_args;

/* The voxel view of `cam`: per pixel the walk of the ray (org = cam->position, dir = the
 * G-buffer caster's primary ray of the pixel, t_lim = +Inf) through `level`, and the colour of
 * the cell it hits.  8 x 8 pixels per wave, K4's screen tiling.
 * VCT_EINVAL, with nothing written: NULL cam or args; a camera or frame size outside the
 * "G-buffer input rule" (near_plane / far_plane are checked by it and otherwise unused);
 * linear4, rgba8 and hit4 all NULL; a misaligned pointer (linear4, hit4: 16 bytes; rgba8: 4;
 * cells: 8); level > L; a mode outside VCT_VOXVIEW_*; ALBEDO or NORMAL with level != 0.
 * VCT_ESTATE when the mode's state is missing.  Queued on the ctx stream; device 0 of a
 * vct_create_multi context. */
vct_status vct_voxel_view_device(vct_ctx* ctx, const vct_camera* cam, const vct_voxel_view_args* args);

#ifdef __cplusplus
}
#endif
#endif /* VCT_VOXVIEW_H */
