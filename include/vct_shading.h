/*
 * vct_shading.h — the shading G-buffer: smooth normals, normal and specular maps, a roughness
 * and a Ks per material.  An additive extension of include/vct.h (which includes this file;
 * VCT_ABI_VERSION stays 1).
 *
 * vct_gbuffer_raster_device writes the face normal of the hit triangle, Kd x map_Kd and one
 * roughness for the whole frame.  The calls here keep a per-triangle record of the vertex
 * attributes the loader already reads (Vertex::Normal, TexCoords, Tangent, Bitangent) and a
 * material table, and write from them
 *
 *   vct_set_shading             the attribute records and the material table of the current
 *                               static voxelization;
 *   vct_gbuffer_shaded_device   the tile-binned pass with a shading normal, the material's
 *                               roughness in alb4.w, a specular-colour plane Ks x map_Ks, and on
 *                               request the geometric normal, the triangle id and the barycentrics;
 *   vct_specular_tint_device    out.rgb = spec.rgb * ks.rgb, so that every existing composite
 *                               honours Ks without a variant of its own.
 *
 * The hit, pos4, the depth test, the albedo and the background texel are those of
 * vct_gbuffer_raster_device in every bit; the per-pixel rule is include/vct_spec.h "shading
 * attributes".  K4 takes any normal and any per-pixel roughness as data, so nothing downstream
 * changes.  Like vct_voxview.h, the functions are implemented by the HIP library only.
 *
 * Call order:  [vct_set_textures ->] vct_voxelize* -> vct_set_shading
 *              -> vct_gbuffer_shaded_device -> vct_trace_device -> vct_specular_tint_device
 *              -> any composite
 */
#ifndef VCT_SHADING_H
#define VCT_SHADING_H

#ifdef __cplusplus
extern "C" {
#endif

#define VCT_SHADING_NO_ATTR    0xFFFFFFFFu  /* attribute absent */
#define VCT_SHADING_FLIP_GREEN 1u           /* material flag: m.y = -m.y */

typedef struct vct_shading_material {
    float    ks[3];        /* Material::Ks */
    float    roughness;    /* written to alb4.w */
    int32_t  normal_map;   /* index into the vct_set_textures set, or -1 */
    int32_t  specular_map; /* index into the same set, or -1 */
    uint32_t flags;
    uint32_t reserved;     /* must be 0 */
} vct_shading_material;

typedef struct vct_shading_desc {
    const void* verts; uint32_t vertex_stride, n_verts;  /* host, the arrays of the last vct_voxelize* */
    const uint32_t* idx; uint32_t n_idx;
    const uint32_t* tri_material;                        /* NULL = material 0 */
    uint32_t normal_offset, uv_offset, tangent_offset, bitangent_offset; /* bytes; 12 / 24 / 32 / 44 in Vertex */
    const vct_shading_material* materials; uint32_t n_materials;
} vct_shading_desc;

/* Builds the per-triangle attribute records (triangle t = idx[3t .. 3t+2], the order of the
 * voxelization's triangles) and keeps the material table, both device resident.  Synchronous:
 * the host arrays are free on return.  A NULL desc clears the set.  Any later vct_voxelize* or
 * vct_load_grid drops the set; vct_voxelize_dynamic* does not (the layer's triangles have
 * indices past the set's and shade flat).  The map indices are checked against the texture set
 * of the moment; a later, smaller vct_set_textures makes a map index stale, and a stale map is
 * treated as no map.
 * VCT_ESTATE without a voxelization.  VCT_EINVAL, with the previous set kept: NULL verts, idx
 * or materials, n_materials == 0; n_idx different from the static voxelization's; an index
 * >= n_verts; a present offset that is not 4-byte aligned or runs past vertex_stride (12 bytes
 * for normal, tangent and bitangent, 8 for uv); tri_material[t] >= n_materials; ks not finite,
 * with its sign bit set, or above VCT_COLOR_LIMIT; roughness not finite or outside [0, 1]; a
 * map index below -1 or beyond the current texture set; unknown flag bits; reserved != 0.
 * Vertex attribute contents are data and never a status. */
vct_status vct_set_shading(vct_ctx* ctx, const vct_shading_desc* desc);

/* The tile-binned G-buffer pass with shading attributes (include/vct_spec.h "shading
 * attributes").  Device pointers; pos4, nrm4, alb4, ks4 and geo4 are [h][w][4] float, 16-byte
 * aligned; tri_id is [h][w] uint32 (4-byte aligned), bary2 [h][w][2] float (8-byte aligned).
 * geo4, tri_id and bary2 may be NULL.  `roughness` goes to the background and to hits outside
 * the set (the dynamic layer).
 * VCT_EINVAL, with nothing written: a camera or frame size outside the "G-buffer input rule";
 * a NULL or misaligned pos4, nrm4, alb4 or ks4; a misaligned optional plane.  VCT_ESTATE
 * without a voxelization or without a set.  Queued on the ctx stream (one 4-byte read back,
 * as vct_gbuffer_raster_device). */
vct_status vct_gbuffer_shaded_device(vct_ctx* ctx, const vct_camera* cam, uint32_t w, uint32_t h, float roughness,
                                     float* pos4, float* nrm4, float* alb4, float* ks4,
                                     float* geo4 /*NULL ok*/, uint32_t* tri_id /*NULL ok*/, float* bary2 /*NULL ok*/);

/* out.rgb = spec.rgb * ks.rgb, out.a = spec.a, per pixel; out4 may be spec4.  Contents are
 * data (NaN and Inf carry through).  VCT_EINVAL: a NULL or misaligned (16 bytes) pointer,
 * w * h == 0 or above 2^31 - 1.  Queued on the ctx stream; needs no voxelization. */
vct_status vct_specular_tint_device(vct_ctx* ctx, const float* spec4, const float* ks4, uint32_t w, uint32_t h,
                                    float* out4);

#ifdef __cplusplus
}
#endif
#endif /* VCT_SHADING_H */
