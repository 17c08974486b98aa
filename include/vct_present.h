/*
 * vct_present.h — the HDR present: a luminance meter, an auto-exposure that adapts over time and
 * never leaves the device, bloom, a choice of tone curve and transfer function, and dithered
 * quantisation.  An additive extension of include/vct.h (which includes this file;
 * VCT_ABI_VERSION stays 1).
 *
 * Every composite presents with Reinhard, gamma 1/2.2 and 8 bits at an exposure of 1 (tone01 and
 * quant8 of csrc/vct_view.h).  The calls here are image-space passes over ANY composite's
 * out_linear4, as vct_specular_tint_device and vct_fog_apply_device are:
 *
 *   vct_luminance_meter_device   a histogram of the frame's luminance, 16 bins per stop;
 *   vct_exposure_update_device   histogram -> a 16-byte exposure record on the device, blended
 *                                towards the metered target from the previous record;
 *   vct_bloom_device             what exceeds a threshold, down a chain of 2 x 2 boxes and back up;
 *   vct_present_device           exposure, bloom, curve, transfer, quantisation -> a display-
 *                                referred float frame and / or RGBA8.
 *
 * All four are stateless, need no voxelization, are queued on the ctx stream and read nothing
 * back: the exposure is produced and consumed on the device.  On a vct_create_multi context
 * device 0 runs them.  The arithmetic is include/vct_spec.h "present"; tests/present_ref.py
 * restates it.  Like vct_shading.h, the functions are implemented by the HIP library only.
 *
 * Call order:  any composite (out_linear4) [-> vct_fog_apply_device, vct_sky_background_device]
 *              -> vct_luminance_meter_device -> vct_exposure_update_device
 *              -> vct_bloom_device -> vct_present_device
 */
#ifndef VCT_PRESENT_H
#define VCT_PRESENT_H

#ifdef __cplusplus
extern "C" {
#endif

#define VCT_PRESENT_BINS      512u    /* hist[]: 16 bins per stop over 2^-16 .. 2^16 */
#define VCT_PRESENT_MAX_DIM   16384u  /* width and height of a frame */
#define VCT_BLOOM_MAX_LEVELS  8u

#define VCT_CURVE_REINHARD        0u  /* v / (1 + v) */
#define VCT_CURVE_REINHARD_WHITE  1u  /* v (1 + v / W^2) / (1 + v), W = params.white */
#define VCT_CURVE_ACES            2u  /* the Narkowicz fit */
#define VCT_CURVE_CLAMP           3u
#define VCT_TRANSFER_GAMMA22      0u  /* powf(v, VCT_INV_GAMMA), as every composite */
#define VCT_TRANSFER_SRGB         1u  /* the piecewise sRGB function */

/* Device record, 16 bytes, 4-byte aligned: the only place the exposure lives. */
typedef struct vct_exposure_state {
    float    exposure;        /* what vct_bloom_device and vct_present_device multiply by */
    float    target;          /* the metered exposure of this frame, before the blend */
    float    mean_luminance;  /* the trimmed mean's bin centre; 0 when nothing was counted */
    uint32_t counted;         /* counts[0] of the frame */
} vct_exposure_state;

typedef struct vct_exposure_params {
    float    key_value;       /* target = key_value / mean luminance */
    float    min_exposure, max_exposure;
    uint32_t low_permille, high_permille;   /* shares of the counted pixels trimmed from either end */
    float    rate_up, rate_down;            /* in [0, 1]: 1 - exp(-dt * speed), computed by the host */
    uint32_t reserved;        /* must be 0 */
} vct_exposure_params;

typedef struct vct_bloom_params {
    float    threshold;       /* of the exposed luminance, finite and >= 0 */
    uint32_t levels;          /* 1 .. VCT_BLOOM_MAX_LEVELS; the chain ends at a 1 x 1 level */
    float    exposure;        /* used when no exposure record is given */
    uint32_t reserved;        /* must be 0 */
} vct_bloom_params;

typedef struct vct_present_params {
    uint32_t curve;           /* VCT_CURVE_* */
    uint32_t transfer;        /* VCT_TRANSFER_* */
    uint32_t dither;          /* 0: quant8 as every composite; 1: the 4 x 4 Bayer table */
    float    exposure;        /* used when no exposure record is given */
    float    white;           /* W of VCT_CURVE_REINHARD_WHITE */
    float    bloom_intensity; /* used when a bloom plane is given */
    uint32_t reserved[2];     /* must be 0 */
} vct_present_params;

/* All four calls: VCT_EINVAL, with nothing written, for a NULL ctx, a NULL or misaligned required
 * buffer (16 bytes for float4 planes and the bloom scratch, 4 for hist, counts and the records), a
 * width or height of 0 or above VCT_PRESENT_MAX_DIM, and a parameter outside its rule.  Pixel,
 * histogram and record contents are device data and never a status. */

/* hist[VCT_PRESENT_BINS] and counts[4] = {counted, under, over, rejected} of linear4 ([h][w][4]
 * float), both written, not accumulated.  A pixel with alpha == 0 is skipped. */
vct_status vct_luminance_meter_device(vct_ctx* ctx, const float* linear4, uint32_t w, uint32_t h,
                                      uint32_t* hist, uint32_t* counts);

/* One small kernel: hist, counts and the previous record (NULL: none) -> out_state.  prev_state
 * and out_state may be the same record.  Parameter rule: key_value, min_exposure <= max_exposure
 * finite, > 0 and <= 2^64; low_permille + high_permille < 1000; rates finite and in [0, 1];
 * reserved == 0. */
vct_status vct_exposure_update_device(vct_ctx* ctx, const uint32_t* hist, const uint32_t* counts,
                                      const vct_exposure_params* params,
                                      const vct_exposure_state* prev_state /*device, NULL ok*/,
                                      vct_exposure_state* out_state /*device*/);

/* Bytes of the scratch of vct_bloom_device for a w x h frame: the levels 1 .. L back to back,
 * level k a [h_k][w_k][4] float plane with w_k = ceil(w_{k-1} / 2) (w_0 = w), L = the first of
 * `levels` and the level that is 1 x 1.  VCT_EINVAL: a size or `levels` outside its rule, NULL bytes. */
vct_status vct_bloom_scratch_bytes(uint32_t w, uint32_t h, uint32_t levels, size_t* bytes);

/* Prefilter, down chain and up chain.  On return (in stream order) level k of the scratch holds
 * U_k; level 1, at the scratch's start, is the half-resolution plane vct_present_device takes.
 * The exposure is exposure_state->exposure when a record is given, else params->exposure (finite,
 * > 0, <= 2^64).  VCT_EINVAL also for scratch_bytes below vct_bloom_scratch_bytes. */
vct_status vct_bloom_device(vct_ctx* ctx, const float* linear4, uint32_t w, uint32_t h,
                            const vct_bloom_params* params, const vct_exposure_state* exposure_state /*device, NULL ok*/,
                            float* scratch, size_t scratch_bytes);

/* out_display4 ([h][w][4] float: the curve's output, alpha copied) and / or out_rgba8 ([h][w]
 * uint32, alpha 255); at least one.  bloom_half4: level 1 of vct_bloom_device's scratch for the
 * same w x h, or NULL.  Parameter rule: curve, transfer and dither known; exposure as above when
 * no record is given; white and white * white finite and > 0 under VCT_CURVE_REINHARD_WHITE; bloom_intensity finite
 * and >= 0 when bloom_half4 is given; reserved == 0.  out_display4 may be linear4. */
vct_status vct_present_device(vct_ctx* ctx, const float* linear4, uint32_t w, uint32_t h,
                              const vct_present_params* params, const vct_exposure_state* exposure_state /*device, NULL ok*/,
                              const float* bloom_half4 /*NULL ok*/, float* out_display4 /*NULL ok*/,
                              uint32_t* out_rgba8 /*NULL ok*/);

#ifdef __cplusplus
}
#endif
#endif /* VCT_PRESENT_H */
