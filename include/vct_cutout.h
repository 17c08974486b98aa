/*
 * vct_cutout.h — alpha-cutout materials: a binary opacity mask honoured by K1 and by a G-buffer
 * pass.  An additive extension of include/vct.h (which includes this file; VCT_ABI_VERSION
 * stays 1).
 *
 * Foliage, chains, grilles and fabric edges are textured quads whose shape lives in an opacity
 * mask (map_d, or the alpha channel of map_Kd).  Everything downstream of K1 and the G-buffer
 * consumes only the occupancy bits, level 0 and the G-buffer planes, so honouring the mask in
 * these two places is enough: K2's shadow walk, the cones, the sky, the fog and the bounces see
 * the holes with no change.
 *
 *   vct_voxelize_cutout[_device]  vct_voxelize_textured[_device] with a per-material cutout
 *                                 table: a (triangle, voxel) pair whose point is not covered
 *                                 adds nothing;
 *   vct_gbuffer_cutout_device     the tile-binned pass over accepted candidates only, writing the
 *                                 flat records of vct_gbuffer_raster_device (ks4 == NULL) or the
 *                                 shaded records of vct_gbuffer_shaded_device;
 *   vct_cutout_materials          the masked materials of the current mesh.
 *
 * The rule is include/vct_spec.h "cutouts".  There is no blending, partial opacity or
 * refraction.  vct_gbuffer_raycast_device, vct_gbuffer_raster_device and
 * vct_gbuffer_shaded_device ignore the table: on a cutout mesh they still write the solid frame.
 * Like vct_shading.h, the functions are implemented by the HIP library only.
 *
 * Call order:  vct_set_textures -> vct_voxelize_cutout* [-> vct_set_shading]
 *              -> vct_gbuffer_cutout_device -> the trace and composites as before
 */
#ifndef VCT_CUTOUT_H
#define VCT_CUTOUT_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vct_cutout {
    int32_t  map;      /* vct_set_textures index of the mask, -1 = opaque        */
    uint32_t channel;  /* 0..3 = r, g, b, a of that texture                      */
    float    cutoff;   /* covered where M >= cutoff; finite, 0 < cutoff <= 1     */
    uint32_t reserved; /* 0                                                      */
} vct_cutout;

/* K1 with cutouts.  Every argument but material_cutout is vct_voxelize_textured's, with its
 * rules and statuses; material_map may be NULL (no diffuse maps).  material_cutout is HOST
 * memory in both forms, n_materials entries, NULL = every material opaque (the call is then
 * vct_voxelize_textured / vct_voxelize).  The table is checked before any launch.  VCT_EINVAL,
 * with the context -- the previous grid and mesh included -- left exactly as it was: map < -1 or
 * >= the texture count; channel > 3; a cutoff that is not finite or outside 0 < cutoff <= 1;
 * reserved != 0; a table with n_materials == 0.
 * One rule is stricter than vct_voxelize_textured's: the table is indexed by the material, so
 * with a table that masks a material a tri_material[t] >= n_materials is always the index
 * error of K1 (VCT_EINVAL, the grid refused), also where material_kd4 and material_map are NULL.
 * A masked triangle whose vertex record holds no TexCoords (uv_offset not a multiple of 4, or
 * uv_offset + 8 > vertex_stride; legal only while material_map is NULL) is opaque.
 * The context keeps the table with the mesh: any later vct_voxelize* or vct_load_grid drops it,
 * vct_voxelize_dynamic* keeps it (the layer's triangles are opaque). */
vct_status vct_voxelize_cutout(vct_ctx* ctx, const void* verts, uint32_t vertex_stride, uint32_t n_verts,
                               const uint32_t* idx, uint32_t n_idx, const uint32_t* tri_material,
                               const float* material_kd4, const int32_t* material_map /*NULL ok*/,
                               const vct_cutout* material_cutout /*HOST, NULL = all opaque*/,
                               uint32_t n_materials, uint32_t uv_offset);
/* The same on device-resident arrays (alignment as vct_voxelize_textured_device);
 * material_cutout stays a host pointer. */
vct_status vct_voxelize_cutout_device(vct_ctx* ctx, const void* verts, uint32_t vertex_stride, uint32_t n_verts,
                                      const uint32_t* idx, uint32_t n_idx, const uint32_t* tri_material,
                                      const float* material_kd4, const int32_t* material_map /*NULL ok*/,
                                      const vct_cutout* material_cutout /*HOST, NULL = all opaque*/,
                                      uint32_t n_materials, uint32_t uv_offset);

/* The tile-binned G-buffer pass over accepted candidates (include/vct_spec.h "cutouts").
 * ks4 == NULL: the flat records of vct_gbuffer_raster_device, and geo4, tri_id and bary2 must be
 * NULL too.  ks4 != NULL: the shaded records of vct_gbuffer_shaded_device, which needs a shading
 * set (VCT_ESTATE without one); geo4, tri_id and bary2 may each be NULL.  Without a cutout mesh
 * the planes equal those calls' in every bit.  A mask index made stale by a later, smaller
 * vct_set_textures is no mask.  The camera rule, the alignments and the NULL rules are
 * vct_gbuffer_shaded_device's: VCT_EINVAL with nothing written.  VCT_ESTATE without a
 * voxelization.  Queued on the ctx stream (one 4-byte read back). */
vct_status vct_gbuffer_cutout_device(vct_ctx* ctx, const vct_camera* cam, uint32_t w, uint32_t h, float roughness,
                                     float* pos4, float* nrm4, float* alb4, float* ks4 /*NULL: flat records*/,
                                     float* geo4 /*NULL ok*/, uint32_t* tri_id /*NULL ok*/, float* bary2 /*NULL ok*/);

/* Masked materials of the current mesh whose triangles can be cut (0: none, no cutout mesh, or
 * a vertex record without TexCoords). */
uint32_t vct_cutout_materials(const vct_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* VCT_CUTOUT_H */
