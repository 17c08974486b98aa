/*
 * vct_emission.h — emissive surfaces: an additive extension of include/vct.h (which
 * includes this file; VCT_ABI_VERSION stays 1).
 *
 * Every light of vct_inject_directional and vct_inject_lights is an analytic direction or
 * point.  The functions here let a surface glow: a material gets an emitted radiance Ke,
 * the triangles that carry it are voxelized into an emission grid E (K1's exact 13-axis
 * test over the emitter triangles; per voxel the average of Ke over all triangles of the
 * mesh that touch it, exactly as the albedo is the average of Kd), E is added into the
 * level-0 radiance, and from there the mips spread it: K4, the bounces and the shadow cones
 * see it with no sampling of their own.  vct_composite_emissive_device shows the emitter
 * itself (include/vct_spec.h "emissive surfaces" has the exact arithmetic).
 *
 * They live in their own header for the reason vct_bounce.h, vct_lights.h and vct_shadow.h
 * do: vct.h's text is the list of symbols every implementation of the boundary exports,
 * and these are implemented by the HIP library only (the reference's Material holds Ka, Kd
 * and Ks, no Ke).
 *
 * Call order:  vct_voxelize*  ->  vct_voxelize_emission*  ->  vct_inject_directional /
 *              vct_inject_lights  ->  vct_inject_emission  ->  vct_build_mips
 *              [-> vct_inject_bounces]  ->  vct_trace*  [-> vct_shadow_cones_device]
 *              ->  vct_composite_emissive_device
 *
 * The emission grid belongs to the voxelization it was built on: every vct_voxelize* call
 * (a failing one included) and every vct_load_grid empties it, and vct_save_grid does not
 * store it.  A context that never calls these functions allocates nothing for them.
 */
#ifndef VCT_EMISSION_H
#define VCT_EMISSION_H

#ifdef __cplusplus
extern "C" {
#endif

/* Builds the context's emission grid E from emitter triangles (host arrays; layout and
 * meaning of verts / vertex_stride / idx / tri_material as vct_voxelize).  material_ke4 =
 * [n_materials][4] floats, Ke.rgb of each material (.a is not read); tri_material = NULL
 * means material 0 for every triangle.  The intended input is the voxelized mesh itself,
 * or a subset of its triangles: a hit in a voxel the voxelization left empty is dropped.
 * A triangle whose Ke is (0,0,0) costs nothing.  Does not touch the voxel grid, level 0 or
 * the mips, and replaces the previous emission grid.
 * VCT_ESTATE before a successful voxelization.  VCT_EINVAL: NULL material_ke4, NULL verts /
 * idx with n_idx > 0, n_idx not a multiple of 3, a bad vertex_stride, a vertex or material
 * index out of range, or a Ke component of a material some triangle uses that is not
 * finite, has its sign bit set (-0.0f included) or is >= VCT_KD_LIMIT (checked before any
 * launch).  After any error the context has an empty emission grid; the voxel grid stays
 * usable.  Vertices follow the K1 input rule: any finite vertex is legal, a triangle with a
 * non-finite q is skipped.
 * Waits for the ctx stream once, to read the candidate count, the number of occupied
 * voxels and the error word back, and once more before it returns (its staging buffers are
 * freed).  On a vct_create_multi context device 0 holds the emission grid. */
vct_status vct_voxelize_emission(vct_ctx* ctx, const void* verts, uint32_t vertex_stride, uint32_t n_verts,
                                 const uint32_t* idx, uint32_t n_idx, const uint32_t* tri_material,
                                 const float* material_ke4, uint32_t n_materials);

/* The same on device-resident arrays (alignment as vct_voxelize_device: material_ke4 16
 * bytes, the others 4; a misaligned pointer is VCT_EINVAL).  Ke is checked by the setup
 * kernel.  Waits for the ctx stream once, as above; the rest of the build is queued. */
vct_status vct_voxelize_emission_device(vct_ctx* ctx, const void* verts, uint32_t vertex_stride, uint32_t n_verts,
                                        const uint32_t* idx, uint32_t n_idx, const uint32_t* tri_material,
                                        const float* material_ke4, uint32_t n_materials);

/* Emissive voxels of the emission grid (0 for an empty one: never built for this
 * voxelization, emptied, or built from emitters that touch no occupied voxel).  The first
 * call after a build waits for the ctx stream to read the count back.  VCT_ESTATE before a
 * voxelization. */
vct_status vct_emission_voxels(vct_ctx* ctx, uint32_t* n_emissive);

/* The emission grid, dense: host_rgba = [n^3][4] floats, linear-Z; (E.rgb, 1) at the emissive
 * voxels, +0 in all four channels elsewhere.  Waits for the ctx stream.  VCT_ESTATE before
 * a voxelization. */
vct_status vct_download_emission(vct_ctx* ctx, float* host_rgba);

/* Level 0 += scale * E at every emissive voxel (one multiply, one add per channel; alpha
 * untouched).  scale must be finite, have a clear sign bit and be <=
 * VCT_EMISSION_SCALE_LIMIT, else VCT_EINVAL with nothing changed.
 * VCT_ESTATE: before a voxelization; without a level 0 (of any origin: inject, light list,
 * upload, device copy); a second call on the same level 0 (the emitters would count twice);
 * a call after vct_inject_bounces on this level 0 (the bounce's L0 must already hold the
 * emission).  Every new level 0 re-arms it.
 * Level 0 stays nonzero exactly where it was (emissive voxels are occupied), so the next
 * vct_build_mips after a K2 may still be a relight build; the mips are not built afterwards.
 * With an empty emission grid the call succeeds and changes nothing, not even that state.
 * Queued on the ctx stream; never waits for the device.  On a vct_create_multi context
 * device 0 adds; the result reaches the other devices with vct_build_mips. */
vct_status vct_inject_emission(vct_ctx* ctx, float scale);

/* vct_composite_shadowed_device plus the emitter itself:
 *     final = ((direct + albedo * diffuse) + spec) + scale * Em
 * with Em = E of the voxel that holds the pixel's position (+0 for a voxel that does not
 * emit, a position outside the grid and a background pixel).  vis = NULL: every light takes
 * the hard voxel walk, as in vct_composite_lights_device; with an empty emission grid or
 * scale = +0 the output then equals that function's bit for bit.  scale as for
 * vct_inject_emission; every other precondition and output is
 * vct_composite_shadowed_device's.  The hard walks of vis = NULL start by the "shadow-walk
 * receiver rule" of vct_spec.h, as vct_composite_lights_device's do. */
vct_status vct_composite_emissive_device(vct_ctx* ctx, const float* pos4, const float* nrm4, const float* alb4,
                                         const float* diffuse4, const float* spec4,
                                         uint32_t width, uint32_t height,
                                         const vct_light* lights, uint32_t n_lights, const float* vis,
                                         float scale, float* out_linear4, uint32_t* out_rgba8);

#ifdef __cplusplus
}
#endif
#endif /* VCT_EMISSION_H */
