/*
 * vct_objects.h — dynamic objects: an additive extension of include/vct.h (which includes this
 * file after vct_dynamic.h; VCT_ABI_VERSION stays 1).
 *
 * vct_voxelize_dynamic* keeps ONE layer of world-space triangles and replaces all of it with
 * every call.  The functions here keep a SET of rigid objects: each is registered once as an
 * object-space mesh, placed by a matrix that may already live on the device, and an update
 * names the objects that moved.  Only those are retracted and voxelized again; every other
 * object's records stay.  K1's state is integer sums accumulated with order-independent
 * atomics, so retracting object k alone is as exact as retracting the whole layer;
 * include/vct_spec.h "dynamic objects" states the equality and the one new piece of
 * arithmetic, the transform rule.
 *
 * They live in their own header for the reason vct_dynamic.h does: vct.h's text is the list of
 * symbols every implementation of the boundary exports, and these are implemented by the HIP
 * library only.
 *
 * Call order:  vct_voxelize* (the static scene, once)
 *              vct_objects_define (once; every object starts hidden)
 *              per frame in which an object moved:
 *                  vct_objects_update* (the moved ones) -> vct_inject_* -> vct_build_mips -> vct_trace*
 *
 * The set
 *   vct_objects_define copies the meshes to the device (packed positions, indices, material
 *   ids), gives every object a fixed triangle range behind the static triangles, in definition
 *   order, and leaves every object hidden: after a successful define the grid equals the static
 *   grid.  n_objects == 0 removes the set: its contribution is retracted and the grid is the
 *   static grid again.  Defining over an existing set replaces it in the same way.  The set
 *   takes Kd materials only, one table for the whole set (material_kd4, or NULL for albedo 1).
 * Equality
 *   Let S be the static mesh, O_k the objects in definition order and P_k the last pose given
 *   for object k.  After any sequence of define / update calls the context equals, bit for bit,
 *   the context after vct_voxelize(union(S, T(O_0, P_0), T(O_1, P_1), ...)): K1's sums and
 *   counts, albedo / occupancy and normals, the occupied set, vct_bounce_sources, every inject,
 *   every mip face, K4, the marches and every composite.  T of a hidden object is its triangles
 *   with every vertex NaN: K1's input rule skips them.  A voxel that only a moved or hidden
 *   object occupied is empty again in every respect: an all-zero record, zero albedo and
 *   normal, a +0 level-0 texel.
 * G-buffer
 *   vct_gbuffer_raycast_device and vct_gbuffer_raster_device see the static triangles, then
 *   object 0's, object 1's, ... in that index order (ties go to the lower index); a hidden
 *   object's are zero triangles, which no ray hits.  The set's triangles shade flat and are
 *   opaque: a live shading set and cutout table are carried over every update.
 * The transform rule
 *   float32, one rounding per operation, no fused multiply-add:
 *       x' = ((m[0] x + m[4] y) + m[8]  z) + m[12]
 *       y' = ((m[1] x + m[5] y) + m[9]  z) + m[13]
 *       z' = ((m[2] x + m[6] y) + m[10] z) + m[14]
 *   m[3], m[7], m[11] and m[15] are not read.  Matrix contents are device data and never a
 *   status: any matrix is legal, and a non-finite result makes the triangle a skipped one under
 *   K1's input rule.  (An identity matrix therefore maps -0.0f to +0.0f, and an infinite
 *   coordinate makes the vertex's other two coordinates NaN: 0 x inf.)
 * Updates
 *   An update names n distinct objects and gives each a pose (poses[j] belongs to ids[j]).
 *   n == 0 is VCT_OK and touches nothing.  Otherwise the call invalidates what
 *   vct_voxelize_dynamic invalidates: level 0, the mips, the bounce / emission / sky marks, the
 *   emission grid and the bounce source list; the next vct_build_mips is a full build.
 * Errors
 *   All are found on the host before any launch, are VCT_EINVAL, and leave the context, the set
 *   and the marks exactly as they were: NULL arrays with non-zero counts, vertex_stride < 12 or
 *   not a multiple of 4, n_idx not a multiple of 3, n_objects > VCT_MAX_OBJECTS, a total
 *   triangle count that does not fit uint32 together with the static mesh, material_kd4 with
 *   n_materials == 0, a Kd that breaks K1's rule, a vertex or material index out of range, an
 *   id >= n_objects or named twice in one update, visible > 1 or reserved != 0 in the host form
 *   (the device form reads visible != 0 and ignores reserved), a device pose pointer that is not
 *   16-byte aligned.
 * State
 *   Before a successful vct_voxelize* / vct_load_grid every call is VCT_ESTATE.  A new
 *   vct_voxelize* / vct_load_grid drops the set: the grid it leaves is the static grid, and an
 *   update is VCT_ESTATE until the set is defined again.  The set and the single layer exclude
 *   each other: vct_objects_define with a layer in place, and vct_voxelize_dynamic* with a set
 *   defined, are VCT_ESTATE; either is removed by its own empty call.  vct_dynamic_voxels is 0
 *   while a set is defined.  vct_save_grid with a set saves the union as a plain grid.
 * Blocking
 *   An update waits for the ctx stream once, at the end: for the redo flag, the stats and K3's
 *   live-block count (a second time in the rare case that the packed accumulators cannot hold
 *   the union and are converted; the result is the same).  vct_objects_define waits for its
 *   uploads.
 * Multi-device
 *   On a vct_create_multi context device 0 runs it, as for the layer.
 */
#ifndef VCT_OBJECTS_H
#define VCT_OBJECTS_H

#ifdef __cplusplus
extern "C" {
#endif

#define VCT_MAX_OBJECTS 4096u

typedef struct vct_object_mesh {      /* HOST arrays, copied by the call */
    const void*     verts;            /* n_verts records of vertex_stride bytes, 3 floats first (object space) */
    uint32_t        vertex_stride, n_verts;
    const uint32_t* idx;              /* n_idx vertex indices, 3 per triangle */
    uint32_t        n_idx;
    const uint32_t* tri_material;     /* per triangle, or NULL (all 0): ids into the set's material table */
} vct_object_mesh;

typedef struct vct_object_pose {      /* 80 bytes, 16-byte aligned in the device form */
    float    m[16];                   /* column-major 4x4 as the host's `model[16]`; m[3], m[7], m[11], m[15] are not read */
    uint32_t visible;                 /* 0 = hidden */
    uint32_t reserved[3];
} vct_object_pose;

typedef struct vct_objects_stats {
    uint32_t n_objects, n_triangles, n_visible;
    uint32_t last_moved_triangles;    /* triangles of the objects named by the last update */
    uint64_t last_candidates;         /* (triangle, voxel) candidates that update walked, retraction + addition */
    uint32_t last_touched_voxels;     /* entries of its fix-up list */
    uint32_t reserved;
} vct_objects_stats;

/* Registers the set (n_objects == 0: removes it).  material_kd4 = n_materials x (Kd.rgb, unused),
 * or NULL (albedo 1). */
vct_status vct_objects_define(vct_ctx* ctx, const vct_object_mesh* meshes, uint32_t n_objects,
                              const float* material_kd4, uint32_t n_materials);

/* Places the n objects ids[j] (HOST array, distinct) by poses[j] (HOST array). */
vct_status vct_objects_update(vct_ctx* ctx, const uint32_t* ids, const vct_object_pose* poses, uint32_t n);

/* The same with poses on the context's device (16-byte aligned); ids stays a HOST array.  The
 * poses may be reused once the call has returned. */
vct_status vct_objects_update_device(vct_ctx* ctx, const uint32_t* ids, const vct_object_pose* poses, uint32_t n);

/* All zero without a set.  Never waits. */
vct_status vct_objects_get_stats(vct_ctx* ctx, vct_objects_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* VCT_OBJECTS_H */
