/*
 * vct_dynamic.h — dynamic objects: an additive extension of include/vct.h (which includes this
 * file; VCT_ABI_VERSION stays 1).
 *
 * vct_voxelize* replaces the whole grid, so moving one object would cost K1 over every
 * triangle of the scene.  The functions here keep one dynamic layer on top of the static
 * grid -- the grid of the last successful vct_voxelize* -- and replace that layer at a cost
 * that follows the layer's triangles and the voxels they touch, not the scene.  K1's state is
 * integer sums accumulated with order-independent atomics, so a triangle's contribution can
 * be added and later subtracted exactly; include/vct_spec.h "dynamic layer" states what that
 * buys: after any sequence of updates the context equals, bit for bit, the context after
 * vct_voxelize of (static triangles followed by the layer's triangles).
 *
 * They live in their own header for the reason vct_bounce.h, vct_lights.h, vct_shadow.h,
 * vct_emission.h and vct_sky.h do: vct.h's text is the list of symbols every implementation of
 * the boundary exports, and these are implemented by the HIP library only.
 *
 * Call order:  vct_voxelize* (the static scene, once)
 *              per frame in which the object moved:
 *                  vct_voxelize_dynamic* -> vct_inject_* -> vct_build_mips -> vct_trace*
 *
 * The layer and the static grid
 *   The context holds at most one layer.  The call replaces the previous layer with the given
 *   triangles; n_idx == 0 removes it.  Before any successful vct_voxelize* (or vct_load_grid)
 *   the call returns VCT_ESTATE.  A new vct_voxelize* or vct_load_grid drops the layer record:
 *   the grid it leaves is then the static grid.  vct_save_grid with a layer in place saves the
 *   union as a plain grid.
 * Equality
 *   After the call, K1's sums and counts (vct_download_accum), albedo / occupancy and normals
 *   (vct_download_voxels), the occupancy and the set of occupied voxels, vct_bounce_sources,
 *   the level 0 any vct_inject_* then writes, every mip face, K4, the shadow and sky marches
 *   and every composite equal what vct_voxelize of the concatenated mesh would leave.  A voxel
 *   that only the removed layer occupied is empty again in every respect: an all-zero record,
 *   zero albedo and normal, a +0 level-0 texel.
 * G-buffer
 *   vct_gbuffer_raycast_device and vct_gbuffer_raster_device see the static triangles, then
 *   the layer's, in that index order (ties go to the lower index): their output is the
 *   concatenated mesh's.
 * Materials
 *   The layer takes Kd materials only (material_kd4, or NULL for albedo 1).  A layer with
 *   diffuse maps is out of scope; over a static scene voxelized with vct_voxelize_textured*
 *   the layer's triangles are untextured.
 * Input rule
 *   K1's (include/vct_spec.h "K1 input rule"): a finite vertex anywhere is legal, a triangle
 *   with a non-finite voxel-unit vertex is skipped, Kd must be finite with |Kd| < VCT_KD_LIMIT.
 * Errors
 *   Found on the host before any launch -- NULL arrays with n_idx > 0, vertex_stride < 12 or
 *   not a multiple of 4, n_idx not a multiple of 3, material_kd4 with n_materials == 0,
 *   misaligned device pointers, and in the host form a Kd that breaks the rule --: VCT_EINVAL,
 *   and the grid and the previous layer stay exactly as they were.
 *   Found by the device -- a vertex or material index out of range, and in the device form a
 *   Kd that breaks the rule --: VCT_EINVAL, and the grid is refused as after a failed
 *   vct_voxelize: VCT_ESTATE from everything that needs a voxelization, this call included,
 *   until a vct_voxelize* succeeds.
 * Invalidation
 *   What vct_voxelize invalidates: level 0, the mips, the bounce / emission / sky marks of
 *   level 0, the emission grid and the bounce source list.  The next vct_build_mips is a full
 *   build.
 * Blocking
 *   Like vct_voxelize_device, the call waits for the ctx stream: once, for the error word and
 *   the counts (a second time in the rare case that the packed accumulators cannot hold the
 *   union and are converted; the result is the same).
 * Multi-device
 *   On a vct_create_multi context device 0 runs it; the changed level 0 reaches the other
 *   devices through the copy vct_build_mips makes.
 */
#ifndef VCT_DYNAMIC_H
#define VCT_DYNAMIC_H

#ifdef __cplusplus
extern "C" {
#endif

/* Host arrays, as vct_voxelize takes them: verts = n_verts records of vertex_stride bytes
 * starting with three floats (position), idx = n_idx vertex indices (three per triangle),
 * tri_material = one material id per triangle or NULL (all 0), material_kd4 = n_materials x
 * (Kd.rgb, unused) or NULL (albedo 1). */
vct_status vct_voxelize_dynamic(vct_ctx* ctx, const void* verts, uint32_t vertex_stride, uint32_t n_verts,
                                const uint32_t* idx, uint32_t n_idx, const uint32_t* tri_material,
                                const float* material_kd4, uint32_t n_materials);

/* The same on device pointers of the context's device, aligned as vct_voxelize_device asks:
 * material_kd4 16-byte, verts, idx and tri_material 4-byte.  The arrays may be reused once the
 * call has returned. */
vct_status vct_voxelize_dynamic_device(vct_ctx* ctx, const void* verts, uint32_t vertex_stride, uint32_t n_verts,
                                       const uint32_t* idx, uint32_t n_idx, const uint32_t* tri_material,
                                       const float* material_kd4, uint32_t n_materials);

/* *n_touched = voxels the current layer hits (0 without a layer).  Never waits. */
vct_status vct_dynamic_voxels(vct_ctx* ctx, uint32_t* n_touched);

#ifdef __cplusplus
}
#endif
#endif /* VCT_DYNAMIC_H */
