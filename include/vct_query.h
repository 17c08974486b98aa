/*
 * vct_query.h — cone queries and an ambient-cube probe grid: an additive extension of
 * include/vct.h (which includes this file; VCT_ABI_VERSION stays 1).
 *
 * Every other consumer of the radiance pyramid is tied to a G-buffer record: K4 traces the
 * fixed diffuse cone set around a pixel's normal and the one cone reflected about it, and the
 * sky, shadow and fog marches read alpha only.  vct_cone_query_device answers the question
 * that is left: what radiance arrives at a given point from a given direction within a given
 * aperture.  It is the primitive for everything that is not an opaque G-buffer pixel: a
 * refraction cone behind glass, a second glossy lobe, particles and transparent surfaces drawn
 * forward, ambient light for objects that are not voxelized, gameplay queries.
 *
 * The probe grid is the first consumer on top of it: a regular grid of ambient-cube probes
 * (six cones per probe, one along each axis direction) built with cone queries, and sampled
 * per point into a plane with the meaning of K4's diffuse4, so any vct_composite_* can light
 * what the G-buffer does not hold.
 *
 * include/vct_spec.h "cone queries" and "probe grid" have the exact arithmetic.  The functions
 * live in their own header for the reason vct_sky.h does: they are implemented by the HIP
 * library only.
 *
 * Call order:  ... vct_build_mips [-> vct_inject_sky / vct_inject_bounces]
 *              -> vct_cone_query_device | vct_probe_build_device
 *              ... per frame: vct_probe_sample_device -> vct_composite_*
 */
#ifndef VCT_QUERY_H
#define VCT_QUERY_H

#ifdef __cplusplus
extern "C" {
#endif

/* One cone.  48 bytes; device arrays of it are 16-byte aligned.  Every float content is legal
 * (non-finite p, d or off, a zero d, a point outside the grid): cone contents are device data
 * and never a status. */
typedef struct vct_cone {
    float p[3];   float tau;     /* world point; tangent of the half aperture, clamped to
                                    [VCT_SPEC_TAU_MIN, VCT_SPEC_TAU_MAX] as the specular cone's */
    float d[3];   float t_lim;   /* direction, used as given (not normalised); the march ends
                                    when t >= t_lim (voxel units; +Inf or NaN: no limit)       */
    float off[3]; float valid;   /* origin offset in voxel units (K4 uses the normal);
                                    valid == 0 (or -0): the cone is skipped                    */
} vct_cone;

typedef struct vct_cone_query_args {
    const vct_cone* cones;           /* device [count], 16-byte aligned                        */
    uint32_t count;
    float* out4;                     /* device [count][4], 16-byte aligned: (c.rgb, a), the
                                        layout of K4's spec4; +0 in all four for a skipped cone */
    uint32_t* steps;                 /* device [count] (4-byte aligned) or NULL: steps per cone */
    unsigned long long* cone_steps;  /* device counter (8-byte aligned), += the steps of the
                                        call, or NULL                                          */
} vct_cone_query_args;

/* Marches every cone of the list through the pyramid: A.5 / A.6's march (K4's), from
 * o = (p - aabb_min) * inv_h + off along d with aperture tau, starting at t = 1, with the one
 * extra stop t >= t_lim.  A cone with p = P, off = N, d = the reflected direction, tau = alb.w
 * and t_lim = +Inf gives the pixel's spec4 bit for bit; the context's diffuse cones, weighted
 * and accumulated in cone order, give diffuse4.
 * One cone per lane, in list order; no cone depends on another, so a permuted list gives the
 * permuted outputs.  An anisotropic two-level step costs up to 48 float4 loads per lane and a
 * wave whose lanes sit on different levels or in different parts of the grid pays for each:
 * ORDER THE CONES SPATIALLY (by origin cell, then aperture) -- the call does not sort.
 * Needs a voxelization and built mips (VCT_ESTATE otherwise).  VCT_EINVAL, with nothing
 * written: NULL args, cones or out4; misaligned cones / out4 (16 bytes), steps (4) or
 * cone_steps (8).  count == 0 is VCT_OK and writes nothing.
 * Queued on the ctx stream; never waits for the device.  On a vct_create_multi context device
 * 0 runs it, on device-0 pointers. */
vct_status vct_cone_query_device(vct_ctx* ctx, const vct_cone_query_args* args);

/* A regular grid of dims[0] x dims[1] x dims[2] probes: probe (i, j, k) stands at
 * origin + (i, j, k) * spacing (world units).  Input rule: origin finite, spacing finite and
 * > 0, each dim in 1 .. VCT_PROBE_MAX_DIM; anything else is VCT_EINVAL with nothing written. */
#define VCT_PROBE_MAX_DIM 256   /* probes per axis */
typedef struct vct_probe_grid {
    float origin[3];
    float spacing;
    uint32_t dims[3];
} vct_probe_grid;

/* Builds the grid: probes = device [dz][dy][dx][6][4] float (16-byte aligned), face f in
 * VCT_FACE_* order = the (c.rgb, a) of the cone query p = the probe's position, off = +0,
 * d = the unit axis of f, tau = VCT_SPEC_TAU_MAX, t_lim = +Inf -- bit for bit what
 * vct_cone_query_device returns for that cone.  state = device [dz][dy][dx] uint32 (4-byte
 * aligned): 1 when the probe lies inside the grid in an empty voxel, else 0 (inside a wall or
 * outside the grid: the sample leaves it out).  cone_steps: as above, or NULL.
 * Both arrays are the caller's; the library keeps nothing (stateless, like the temporal
 * history), so a host may build into one set while a frame samples another.
 * VCT_ESTATE without a voxelization and built mips; VCT_EINVAL, with nothing written: the
 * input rule, NULL grid / probes / state, a misaligned pointer.  Queued on the ctx stream. */
vct_status vct_probe_build_device(vct_ctx* ctx, const vct_probe_grid* grid, float* probes, uint32_t* state,
                                  unsigned long long* cone_steps);

/* Per point m < count with pos4[m].w != 0: the trilinear blend of the valid probes around
 * pos4[m].xyz, evaluated as an ambient cube along nrm4[m].xyz (one face per axis by the sign
 * of n_c, weighted n_c^2, the normal used as given), into out4[m] = (irradiance.rgb,
 * 1 - occlusion) -- the meaning of K4's diffuse4, so every vct_composite_* takes the plane
 * unchanged.  No valid probe around the point: (0, 0, 0, 1) and *misses += 1 (device,
 * 4-byte aligned, or NULL).  A background point (pos.w == 0) gets +0 in all four channels.
 * pos4, nrm4, out4: device [count][4] float, 16-byte aligned.  Needs no grid state.
 * VCT_EINVAL, with nothing written: the input rule, a NULL or misaligned pointer (misses may
 * be NULL).  count == 0 is VCT_OK.  Queued on the ctx stream. */
vct_status vct_probe_sample_device(vct_ctx* ctx, const vct_probe_grid* grid, const float* probes,
                                   const uint32_t* state, const float* pos4, const float* nrm4, uint32_t count,
                                   float* out4, uint32_t* misses);

#ifdef __cplusplus
}
#endif
#endif /* VCT_QUERY_H */
