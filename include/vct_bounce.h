/*
 * vct_bounce.h — light bounces: an additive extension of include/vct.h (which includes
 * this file; VCT_ABI_VERSION stays 1).
 *
 * After K2 and K3 a frame carries direct light plus one indirect bounce, gathered from a
 * grid that holds direct light only: a voxel the light does not reach is +0 in every
 * cone, however brightly its neighbours are lit.  vct_inject_bounces makes the grid carry
 * bounced light: every occupied voxel with a nonzero normal becomes a cone origin, K4's
 * diffuse cone set gathers irradiance I there, and albedo x I is added to the level-0
 * radiance (include/vct_spec.h "light bounces" has the exact arithmetic).
 *
 * The two functions live in their own header because they are implemented by the HIP
 * library only: vct.h's text is the list of symbols that every implementation of the
 * boundary exports (the CPU oracle backend included), and the oracle needs no bounce of
 * its own -- the expected grid is a composition of its trace and mip calls.
 *
 * Call order:  vct_voxelize*  ->  vct_inject_directional  ->  vct_build_mips  ->
 *              vct_inject_bounces(ctx, n)  ->  vct_trace* ...
 */
#ifndef VCT_BOUNCE_H
#define VCT_BOUNCE_H

#ifdef __cplusplus
extern "C" {
#endif

/* n_bounces more light bounces into the level-0 radiance (vct_spec.h "light bounces").
 * Needs vct_voxelize*, a level 0 and built mips (VCT_ESTATE otherwise); leaves the mips
 * built from the result.  n_bounces = 0 is a no-op.  A second call without a new level 0
 * (inject / upload / set_level0 / load) in between is VCT_ESTATE: it would count the
 * direct light twice.
 * Queued on the ctx stream like vct_inject_directional.  The first call after a
 * voxelization (or a load) builds the source list and waits for the ctx stream once, to
 * read the number of sources back; every later call (a relight) queues its kernels and
 * returns.  It never waits for the device or for another stream.
 * On a vct_create_multi context device 0 bounces; the result reaches the other devices
 * with the level-0 peer copy of the final mip build. */
vct_status vct_inject_bounces(vct_ctx* ctx, uint32_t n_bounces);
/* sources of the current voxelization (occupied voxels with a nonzero normal); builds the
 * source list if it is stale (one wait for the ctx stream, as above) */
vct_status vct_bounce_sources(vct_ctx* ctx, uint32_t* n_sources);

#ifdef __cplusplus
}
#endif
#endif /* VCT_BOUNCE_H */
