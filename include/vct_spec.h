/*
 * vct_spec.h — normative constants of the voxel-cone-tracing (VCT) hot path.
 *
 * The reference (fysososo/voxel-based-global-illumination) never implemented the
 * GI stages: `VoxelizationProgram` is an empty subclass
 * (assets/code/program/p_voxelization.h:4-7) and `VoxelizationRenderer::Render`
 * only draws a forward-textured mesh (assets/code/renderer/r_voxelization.cpp:4-35).
 * SURVEY.md Appendix A therefore defines the semantics; this header pins every
 * free parameter of that spec as a literal so that the HIP kernels
 * (voxel-based-global-illumination_amd/csrc) and the CPU oracle (oracle/) read the
 * SAME numbers.  Nothing here is code; it is plain C89-compatible data so the
 * C oracle, the C++ host and the HIP device code can all include it.
 *
 * Units.  All cone / DDA / SAT arithmetic is carried out in level-0 VOXEL units:
 *   q = (p - aabb_min) * inv_h,  inv_h = (float)n / extent   (float divide)
 * so a voxel has edge 1, the grid spans [0, n]^3, level l texel coords are
 * q * 2^-l - 0.5 (GL texel-centre convention).
 *
 * Floating point.  Every translation unit of the path is compiled with
 * -ffp-contract=off.  The only fused multiply-adds are the explicit fmaf()
 * calls that the spec names (trilinear accumulation, level blend, composite,
 * cone-weight accumulation, the log2 polynomial); they are exact on both the
 * host (libm / x86 FMA) and the device (v_fma_f32), so oracle and kernels can
 * agree bit for bit.
 */
#ifndef VCT_SPEC_H
#define VCT_SPEC_H

/* ---- A.6 cone marching ---------------------------------------------------- */
#define VCT_ALPHA_STOP      0.95f        /* stop when a >= 0.95                    */
#define VCT_STEP_SCALE      0.5f         /* t += 0.5 * D                            */
#define VCT_SQRT3           1.7320508f   /* t_max = n * sqrt(3) (voxel units)       */
#define VCT_SPEC_TAU_MIN    0.02f        /* specular tau = clamp(roughness, .02, 1) */
#define VCT_SPEC_TAU_MAX    1.0f
#define VCT_QUERY_MAX_STEPS 4096        /* loop bound of a cone query (> 2*1024*sqrt(3) + 1) */

/* ---- log2 used for the mip level m = log2(D) (D >= 1) ----------------------
 * m = e + 2*s*P(s^2)/ln2 with x = 2^e * f, f in [1/sqrt2, sqrt2], s=(f-1)/(f+1)
 * P(z) = 1 + z/3 + z^2/5 + z^3/7 + z^4/9 (Horner, fmaf).  |err| < 2e-7.      */
#define VCT_LOG2_SQRT2      1.41421354f
#define VCT_INV_LN2         1.44269502f
#define VCT_LOG2_C9         0.111111112f
#define VCT_LOG2_C7         0.142857149f
#define VCT_LOG2_C5         0.200000003f
#define VCT_LOG2_C3         0.333333343f

/* ---- diffuse cone sets ------------------------------------------------------
 * d_k = cn*n + ct*T + cb*B with (T,B) the Duff et al. 2017 branchless ONB of n.
 * Row = (cn, ct, cb, weight).  Weights are cos-theta normalised.               */
#define VCT_TAN30           0.577350259f /* 9-cone and 1-cone half-angle tangent   */
#define VCT_TAN20           0.36397022f  /* 16-cone half-angle tangent             */

/* 9 cones: d0 = n, d_k at 45 deg polar, phi_k = (k-1)*45 deg       */
#define VCT_CONES9(X)                                                   \
    X(1.0f,        0.0f,        0.0f,        0.150221109f)             \
    X(0.707106769f, 0.707106769f, 0.0f,      0.106222361f)             \
    X(0.707106769f, 0.5f,        0.5f,       0.106222361f)             \
    X(0.707106769f, 0.0f,        0.707106769f, 0.106222361f)           \
    X(0.707106769f, -0.5f,       0.5f,       0.106222361f)             \
    X(0.707106769f, -0.707106769f, 0.0f,     0.106222361f)             \
    X(0.707106769f, -0.5f,       -0.5f,      0.106222361f)             \
    X(0.707106769f, 0.0f,        -0.707106769f, 0.106222361f)          \
    X(0.707106769f, 0.5f,        -0.5f,      0.106222361f)

/* 1 cone (config C1): d0 = n, w = 1                                            */
#define VCT_CONES1(X)  X(1.0f, 0.0f, 0.0f, 1.0f)

/* 16 cones (config C5): centre + 5 at 30 deg + 10 at 60 deg (phi offset 18 deg) */
#define VCT_CONES16(X)                                                  \
    X(1.0f,        0.0f,          0.0f,          0.0968042314f)        \
    X(0.866025388f, 0.5f,          0.0f,          0.0838349238f)       \
    X(0.866025388f, 0.154508501f,  0.475528270f,  0.0838349238f)       \
    X(0.866025388f, -0.404508501f, 0.293892622f,  0.0838349238f)       \
    X(0.866025388f, -0.404508501f, -0.293892622f, 0.0838349238f)       \
    X(0.866025388f, 0.154508501f,  -0.475528270f, 0.0838349238f)       \
    X(0.5f,        0.823639095f,  0.267616570f,  0.0484021157f)        \
    X(0.5f,        0.509036958f,  0.700629294f,  0.0484021157f)        \
    X(0.5f,        0.0f,          0.866025388f,  0.0484021157f)        \
    X(0.5f,        -0.509036958f, 0.700629294f,  0.0484021157f)        \
    X(0.5f,        -0.823639095f, 0.267616570f,  0.0484021157f)        \
    X(0.5f,        -0.823639095f, -0.267616570f, 0.0484021157f)        \
    X(0.5f,        -0.509036958f, -0.700629294f, 0.0484021157f)        \
    X(0.5f,        0.0f,          -0.866025388f, 0.0484021157f)        \
    X(0.5f,        0.509036958f,  -0.700629294f, 0.0484021157f)        \
    X(0.5f,        0.823639095f,  -0.267616570f, 0.0484021157f)

#define VCT_MAX_CONES       17           /* 16 diffuse + 1 specular                */

/* ---- A.4 anisotropic faces --------------------------------------------------
 * Face f is the one SAMPLED by cones travelling along that direction; its
 * "front" child is the one a +X-travelling cone meets first (smaller x).      */
#define VCT_FACE_PX 0
#define VCT_FACE_NX 1
#define VCT_FACE_PY 2
#define VCT_FACE_NY 3
#define VCT_FACE_PZ 4
#define VCT_FACE_NZ 5
#define VCT_NUM_FACES 6

/* ---- A.2 voxelization fixed point ------------------------------------------ */
#define VCT_FIXED_ONE       65536.0f     /* round(x * 2^16) into int64 sums        */
#define VCT_FIXED_ONE_D     65536.0
/* K1 input rule (what a finite-or-not mesh means; every implementation restates it):
 *  Candidate range of a triangle on one axis, from mn / mx = fminf / fmaxf of its three q:
 *      lo = (int)ceilf(fminf(fmaxf(mn, -1), n + 1)) - 1,  clamped up to 0
 *      hi = (int)floorf(fmaxf(fminf(mx, n + 1), -1)),     clamped down to n - 1
 *    Both ends are clamped to [-1, n + 1] BEFORE the float -> int conversion, so the
 *    conversion is defined for every finite q however far outside the grid.
 *  Non-finite vertices: a triangle with any non-finite component of q (NaN or +-Inf; tested
 *    on q, so an overflow of (p - g0) * inv_h counts) is skipped.  It has no candidates,
 *    adds nothing to any voxel, and is kept for the G-buffer passes as an all-zero triangle
 *    (zero origin and edges: no ray hits it).  It is not an error.
 *  Kd: each of a triangle's material Kd.r, .g, .b must be finite with |Kd| < VCT_KD_LIMIT =
 *    2^31 / VCT_FIXED_ONE: with a 32-bit count a voxel's int64 sum then cannot overflow,
 *    and (int64)roundf(Kd * 2^16) is defined.  Otherwise the voxelization is an error
 *    (VCT_EINVAL) and the grid is refused afterwards as for an index out of range.
 *    Negative finite Kd is legal.  Kd.a is not read. */
#define VCT_KD_LIMIT        32768.0f

/* K2 input rule (what a light direction and colour mean to the A.3 shadow walk, to
 * vct_inject_directional, vct_composite_device and every light of a list; every implementation
 * restates it):
 *  Direction: len = sqrtf((dx*dx + dy*dy) + dz*dz) in float32 must be finite and > 0, otherwise
 *    the call is an error (VCT_EINVAL).  A non-finite component is therefore refused, and so is
 *    a finite direction whose squared length underflows to 0 or overflows to +inf.  l = d / len
 *    per component (directional lights, and the axis of a spot light).
 *  Walk: per axis a, s_a = sign(l_a) and td_a = 1.0f / fabsf(l_a) (+inf where l_a == 0).  An
 *    axis whose td_a is not finite does not move: s_a = 0 and tm_a = +inf.  That is the axis of
 *    a zero component, as always, and now also of a component with |l_a| <= 2^-128 (a denormal
 *    whose reciprocal overflows), for which (q_a - v_a) * td_a would be 0 * inf = NaN at an
 *    integer q_a.  Under this rule no t of the walk is ever NaN: tm_a starts as a finite
 *    non-negative product or +inf, and only grows by additions of a positive td_a.  The step is
 *    x if tmx <= tmy and tmx <= tmz, else y if tmy <= tmz, else z; at least one component of l
 *    is O(1), so the axis chosen always has a finite t.
 *  Colour: each of color.r, .g, .b must be finite, not negative (-0.0f counts as negative, by
 *    its sign bit) and <= VCT_COLOR_LIMIT, otherwise VCT_EINVAL.  An error leaves level 0 as it
 *    was.  The limit keeps level 0 finite: a voxel's albedo is an average of legal Kd x T, so
 *    |A| < VCT_KD_LIMIT = 2^15; ndl <= |N| |l| plus rounding < 2 for a unit normal; f <= 1 and
 *    V <= 1; at most VCT_MAX_LIGHTS = 2^6 lights are summed.  With color <= 2^105 every
 *    contribution is below 2^15 * 2^105 * 2 = 2^121 and the sum below 2^127 < FLT_MAX:
 *    VCT_COLOR_LIMIT = 2^127 / (VCT_KD_LIMIT * 2 * VCT_MAX_LIGHTS) = 2^105. */
#define VCT_COLOR_LIMIT     4.05648192e31f   /* 2^105 exactly */

/* Shadow-walk receiver rule (what a caller's pixel means to the A.3 shadow walk: the composites
 * vct_composite_device, vct_composite_lights_device, vct_composite_emissive_device with vis NULL,
 * and the hard lights, tan_half 0, of vct_shadow_cones_device; every implementation restates it):
 *  A pixel is legal whenever pos4.w != 0; its q_a = (P_a - g0_a) * inv_h + N_a may be anything a
 *  float32 holds.  The walk from a receiver starts only if
 *      0 <= q_a && q_a < (float)n      in float32, for a = x, y, z.
 *  The compare happens BEFORE any float -> int conversion.  A NaN fails it; -0.0f passes (and
 *  floorf(-0.0f) converts to cell 0).  Otherwise V = 1 and nothing is read: the receiver lies
 *  outside the grid, which no voxel shadows.
 *  Equivalence: for every q_a an int holds (-2^31 <= q_a < 2^31), floorf(q_a) < 0 exactly when
 *  q_a < 0 and floorf(q_a) >= n exactly when q_a >= n (n is an integer), so the test equals
 *  A.3's own "start cell outside the grid gives V = 1" on v_a = (int)floorf(q_a) bit for bit:
 *  no result that was defined changes.  What the rule adds is a result for the q no int
 *  holds -- NaN, +-inf, |q_a| >= 2^31 -- where (int)floorf(q_a) is undefined in C and differs
 *  between machines (x86 gives INT_MIN for all of them; gfx950 saturates and turns NaN into 0, a
 *  start cell inside the grid, with a tm_a of NaN that loses every <=, so that an axis the walk
 *  needs can never move).
 *  A soft light (tan_half != 0) keeps what "shadow cones" gives: for a receiver with a NaN
 *  component, or one too far out for t <= t_max to bring p back (+-inf, 1e30, 2^31), step 1
 *  ends the cone before its first sample (a NaN fails the compares of "p outside [0, n]^3"):
 *  0 steps, a = +0, V = 1.  The hard and the soft path of one call therefore agree on every
 *  such receiver.  (A receiver just outside the grid whose cone re-enters it marches, as
 *  before; its hard walk gives 1, as before.)
 *  K2's receivers (an occupied voxel's centre plus its K1 normal) are finite and inside the
 *  test's int range by the K1 input rule; K2 keeps A.3's test on the converted cell. */
/* "environment sky" (below): the largest texel of a map and the largest scale of a record, so
 * that Env <= 2^104 (1 + 2^-21) stays below VCT_COLOR_LIMIT */
#define VCT_ENV_TEXEL_LIMIT 4503599627370496.0f  /* 2^52 exactly */

/* G-buffer input rule (what a camera, a frame size and a mesh mean to vct_gbuffer_raycast_device
 * and vct_gbuffer_raster_device; one rule for both calls; every implementation restates it):
 *  Definition: the brute-force caster defines the result.  Per pixel (x, y), row 0 = top:
 *      tan_half = tanf(zoom_deg * 0.5f * 3.14159265358979f / 180.0f), aspect = (float)w / (float)h
 *      ndx = (2 * (x + 0.5f) / w - 1) * tan_half * aspect,  ndy = (1 - 2 * (y + 0.5f) / h) * tan_half
 *      D = front + ndx * right + ndy * up,  d = D * (1.0f / sqrtf(dot3(D, D)))
 *    The binned pass returns the same three planes bit for bit on every legal input.
 *  Hit selection: t_k = the Moller-Trumbore parameter of triangle k (|det| < 1e-12f, u < 0,
 *    u > 1, v < 0 or u + v > 1 is a miss).  The hit is the smallest t_k > 0 over ALL triangles,
 *    the lower index on equal t.  Only then depth = t * dot3(d, front) is tested: the pixel is
 *    background if there is no hit, depth < near_plane or depth > far_plane.  A hit nearer
 *    than near_plane (or farther than far_plane) therefore hides what lies behind it; it is
 *    not skipped in favour of the next one.
 *  Camera (anything else is VCT_EINVAL, with nothing written to the three planes):
 *    position: three finite floats.
 *    front, up, right: finite, and orthonormal to VCT_GBUF_ORTHO_EPS = 2^-20: with the dot
 *      products taken in double, |a.a - 1| <= eps for each of the three and |a.b| <= eps for
 *      each of the three pairs.  Handedness is not tested (a mirrored basis mirrors the frame).
 *      A vct.camera.Camera (float64-normalised, rounded to float32) is within 1.1e-7 and the
 *      float32 GLM camera of the host within 2.3e-7 at every yaw and pitch.
 *    zoom_deg: VCT_GBUF_ZOOM_MIN < zoom_deg < VCT_GBUF_ZOOM_MAX (2^-10 and 179 degrees; NaN
 *      fails both), so tan_half is finite and positive.
 *    near_plane, far_plane: finite, 0 <= near_plane <= far_plane (equal is legal).
 *    w, h: 1 <= w, h <= VCT_GBUF_MAX_DIM = 2^14 each (at most 2^20 bins and 2^28 pixels).
 *    focal length: with s = h / (2 tan_half) (pixels per unit of tangent, the same on both
 *      axes) and M = 1 + tan_half * (1 + w / h) (a bound of |D|), in double from the float
 *      tan_half:  s * M * M <= VCT_GBUF_FOCAL_LIMIT = 2^17.  This is what keeps the float32
 *      projection of the binned pass within a quarter of a pixel.
 *  Triangles are device data, never a status: any finite vertices (1e18 included), zero-area
 *    triangles and the all-zero record of a K1-skipped triangle ("K1 input rule") do what the
 *    Moller-Trumbore test above says in float32; an all-zero record is never hit. */
#define VCT_GBUF_ORTHO_EPS    9.5367431640625e-07   /* 2^-20 (double)  */
#define VCT_GBUF_ZOOM_MIN     0.0009765625f         /* 2^-10 degrees   */
#define VCT_GBUF_ZOOM_MAX     179.0f
#define VCT_GBUF_MAX_DIM      16384u                /* 2^14            */
#define VCT_GBUF_FOCAL_LIMIT  131072.0              /* 2^17 (double)   */

/* ---- diffuse maps (albedo = Kd x diffuse map; SURVEY 8a Model::loadMaterials) --
 * The reference loads a material's map_Kd with stbi_load(path, .., 0), uploads it
 * as glTexImage2D(GL_RED | GL_RGB | GL_RGBA, GL_UNSIGNED_BYTE) and samples it with
 * GL_REPEAT wrap and GL_LINEAR magnification (model.cpp:150-226, :212-216) at the
 * assimp-flipped UV (aiProcess_FlipUVs, model.cpp:24: v' = 1 - v).
 *  Texture: W x H RGBA8, row 0 = the image's first (top) row = GL's t = 0 row;
 *    1 / 3 channels expand as GL_RED / GL_RGB sample: (r,0,0,255) / (r,g,b,255).
 *    (2 channels: the reference leaves `format` uninitialised, model.cpp:200-206;
 *    such a map is refused and the material keeps Kd.)
 *  Texel value c / 255.0f per channel (float division).
 *  T(u, v) for the TexCoords (u, v') of the vertex record (already flipped):
 *    fu = u - floorf(u), fv = v' - floorf(v')          (non-finite coordinate -> 0)
 *    s = fu * W - 0.5,  t = fv * H - 0.5               (texel-centre convention)
 *    x0 = floorf(s), ax = s - x0, x1 = x0 + 1 (likewise y0, ay, y1), wrapped into
 *    [0, W) / [0, H) (GL_REPEAT; x0 >= -1 and x1 <= W by construction)
 *    lerp(a, b, f) = fmaf(f, b - a, a)
 *    T = lerp(lerp(T[y0][x0], T[y0][x1], ax), lerp(T[y1][x0], T[y1][x1], ax), ay)
 *    rgb only.  Base level only: voxelization and the G-buffer have no screen-space
 *    derivative to pick a GL_LINEAR_MIPMAP_LINEAR level from.
 *  UV of a (triangle, voxel) hit in K1: the voxel centre c projected onto the
 *    triangle's plane, in voxel units (q0, q1, q2 = the vertices):
 *      e1 = q1 - q0, e2 = q2 - q0, w = c - q0, dot = (x*x' + y*y') + z*z'
 *      d11 = e1.e1, d12 = e1.e2, d22 = e2.e2, w1 = w.e1, w2 = w.e2
 *      den = d11*d22 - d12*d12; b1 = b2 = 0 unless den > 0, else
 *      b1 = (d22*w1 - d12*w2) / den, b2 = (d11*w2 - d12*w1) / den
 *      b1 = fmaxf(b1, 0), b2 = fmaxf(b2, 0); if (b1 + b2 > 1) b1 /= s, b2 /= s (s = b1 + b2)
 *    and in the G-buffer: (b1, b2) = the Moller-Trumbore (u, v) of the nearest hit.
 *    uv = fmaf(b2, uv2 - uv0, fmaf(b1, uv1 - uv0, uv0)) per component.
 *  Albedo = Kd.rgb * T.rgb, then (K1) round(albedo * 2^16) into the int64 sums. */
#define VCT_TEX_MAX_DIM     16384u       /* largest texture edge accepted           */

/* ---- multi-GPU screen tiling ---------------------------------- */
#define VCT_TILE            64           /* 64x64-pixel tiles, round-robin by rank */

/* Composite + present:
 *   direct = ((albedo * color) * max(n.l, 0)) * V     V: the K2 DDA shadow walk
 *            from q = (P - g0) * n/E + N (the cone origin) toward l
 *   final  = (direct + albedo * diffuse.rgb) + spec.rgb          (linear)
 *   rgba8  = round(255 * (f / (1 + f))^(1/2.2)) per channel, alpha 255;
 *            background pixels = the reference's clear colour
 *            (glClearColor(0.2, 0.3, 0.3, 1), r_voxelization.cpp:8). */
#define VCT_CLEAR_R         0.2f
#define VCT_CLEAR_G         0.3f
#define VCT_CLEAR_B         0.3f
#define VCT_INV_GAMMA       0.454545468f /* 1 / 2.2 */
/* The voxel view ("voxel view", below) presents through the same step.  Its shade: the hit
 * cell's colour times one literal per entry-face axis, so cubes read as cubes; and the cap of
 * its walk, in steps per cell of an axis. */
#define VCT_VOXVIEW_SHADE_X        0.8f
#define VCT_VOXVIEW_SHADE_Y        1.0f
#define VCT_VOXVIEW_SHADE_Z        0.6f
#define VCT_VOXVIEW_STEPS_PER_CELL 3
/* The HDR present ("present", below): the key of 2^-16 in the luminance meter, (127 - 16) << 4;
 * the sRGB transfer's exponent, 1 / 2.4; and the largest exposure or key value, 2^64. */
#define VCT_PRESENT_KEY0      1776u
#define VCT_SRGB_INV_GAMMA    0.416666657f
#define VCT_EXPOSURE_LIMIT    18446744073709551616.0f

/* ---- light bounces (vct_inject_bounces, include/vct_bounce.h; no new literals) ------
 * L0 = the level-0 radiance at the call (K2's output), A / N = K1's resolved albedo and
 * normal grids, g0, E, n = the grid.
 *  Sources: every occupied voxel whose resolved normal is not (0,0,0).  Occupied voxels
 *    with a zero normal (two-sided thin geometry whose normals cancel) receive no bounce
 *    and keep L0; empty voxels stay +0.
 *  The source at integer voxel (x,y,z) is the G-buffer record
 *      hh  = E / (float)n                                 (float divide)
 *      P_c = g0_c + ((float)x_c + 0.5f) * hh              (multiply, then add; no fma)
 *      P.w = 1, normal = N[v].xyz, albedo = A[v].rgb      (roughness unused)
 *    and the bounce gather is K4 (A.5, A.6) on that record with the context's diffuse
 *    cone set (n_diffuse, aniso) and no specular cone, whatever cfg.specular is.  The
 *    cone origin is therefore (P - g0) * inv_h + N as A.5 computes it from a world
 *    position, not x + 0.5 (the round trip through P is inexact for ~40 % of the voxels
 *    of a 32^3 grid).
 *  One bounce (Jacobi): I_k = K4.diffuse.rgb gathered from the pyramid built from L_k;
 *      L_{k+1}.rgb = L0.rgb + A.rgb * I_k.rgb             (one multiply, one add per channel)
 *      L_{k+1}.a   = L0.a
 *    at every source.  Every bounce adds to L0, never to L_k; no gather sees another
 *    voxel's update of the same bounce (level 0 is not written while the gather runs);
 *    after each bounce the pyramid is rebuilt from L_{k+1}.  Level 0 stays nonzero
 *    exactly at the occupied voxels (alpha), so the relight mip build stays legal.
 *  n_diffuse = 0: I = 0 and L stays L0. */

/* ---- local lights (vct_inject_lights / vct_composite_lights_device, include/vct_lights.h;
 *      no new literals) ------------------------------------------------------------------
 * No fused operation: every step below is one IEEE float op, in the order written; sqrtf
 * and / are correctly rounded, denormals are kept.
 *      dot3(a, b) = (ax*bx + ay*by) + az*bz
 *      inv_h = (float)n / E,  hh = E / (float)n                    (float divides)
 *  Per light, once, on the host:
 *    directional:  l = d / sqrtf(dot3(d, d)) per component, as vct_inject_directional
 *    point, spot:  pL_c   = (position_c - g0_c) * inv_h            (voxel units)
 *                  rv     = range * inv_h
 *                  inv_rr = 1.0f / (rv * rv)
 *                  h2     = hh * hh
 *    spot only:    a        = -(direction / sqrtf(dot3(direction, direction)))
 *                  inv_span = 1.0f / (cos_inner - cos_outer)
 *  Per receiver and per light, in list order.  A receiver is, in K2, an occupied voxel
 *  (x, y, z) with resolved normal N and albedo A, q_c = ((float)x_c + 0.5f) + N_c; in the
 *  composite, a pixel with position P, normal N, albedo A, q_c = (P_c - g0_c) * inv_h + N_c.
 *    directional:  l = the light's l,  f = 1.0f,  t_lim = +inf
 *    point, spot:  d = pL - q,  r2 = dot3(d, d);  the light is skipped unless r2 > 0
 *                  r = sqrtf(r2),  l_c = d_c / r,  t_lim = r
 *                  u = r2 * inv_rr,  w = fmaxf(1.0f - u, 0.0f)
 *                  f = (w * w) / (1.0f + r2 * h2)
 *    spot only:    cd = dot3(l, a)
 *                  s = fminf(fmaxf((cd - cos_outer) * inv_span, 0.0f), 1.0f)
 *                  f = f * (s * s)
 *    ndl = dot3(N, l);  the light is skipped unless ndl > 0 and f > 0.
 *  (f is the physical 1 / (1 + r_world^2) falloff under a window that reaches zero, with a
 *  zero slope, at r_world = range.)
 *  Visibility V: the A.3 shadow walk (vct_device.h dda_visibility; "K2 input rule": an axis
 *  whose td is not finite does not move) from q along l, cell
 *  for cell, with one more end.  t_e is the t at which the current cell was entered: 0 for
 *  the first cell; after a step, the tm value that was the minimum chosen (before td is
 *  added to it).  Before a cell is tested: t_e >= t_lim gives V = 1 (the light is
 *  reached).  A start cell outside the grid gives V = 1 as in A.3; for the composite's receiver
 *  that test is the "shadow-walk receiver rule" (float compares on q, before the conversion).
 *  Sum:  contrib_c = (((A_c * color_c) * ndl) * f) * V
 *        acc = +0;  acc_c = acc_c + contrib_c  for the lights not skipped, in list order
 *    K2 writes (acc, 1) at the voxel; the composite uses direct = acc in
 *    final = (direct + A * D) + S.
 *  One directional light therefore reproduces vct_inject_directional and
 *  vct_composite_device bit for bit (x * 1.0f and +0 + x are exact for x >= 0), and the
 *  order of the list is part of the result. */

/* ---- shadow cones (vct_shadow_cones_device / vct_composite_shadowed_device,
 *      include/vct_shadow.h; no new literals) ---------------------------------------------
 *  Receiver: a pixel with pos.w != 0.  Its q and N, and per light l, f, ndl, t_lim and the
 *  skip rule, are those of "local lights" (the composite receiver), in list order.
 *  tan_half[j] == 0:  V is the "local lights" shadow walk, unchanged (V in {0, 1}).
 *  Otherwise:  tau = fminf(fmaxf(tan_half[j], VCT_SPEC_TAU_MIN), VCT_SPEC_TAU_MAX), and the
 *  march is the alpha component of A.6 with o = q, d = l, a = 0, t = 1, L = log2 n,
 *  t_max = (float)n * VCT_SQRT3:
 *    1. Before each sample, in this order:
 *         end if !(a < VCT_ALPHA_STOP)                     (alpha stop)
 *         end if !(t <= t_max)
 *         end if t >= t_lim                                (the light is reached)
 *         p_c = o_c + d_c * t  (multiply, then add; no fma);  end if p is outside [0, n]^3,
 *         that is unless 0 <= p_c <= n for every c         (left the grid)
 *    2. D = fmaxf(1.0f, (2.0f * tau) * t);  m = fminf(log2(D), (float)L) with the log2 of
 *       VCT_LOG2_*;  l0 = (int)m;  fr = m - (float)l0
 *    3. s = the alpha of D_l0(p, d) exactly as A.5 computes it: texel coordinates
 *       c = p * 2^-l0 - 0.5f (the product is exact), i = floorf(c), w = c - i, the two
 *       weights per axis (1.0f - w, w); faces chosen by d_c >= 0;
 *       face weights d_c * d_c; per corner texel v = fmaf(dz2, Fz, fmaf(dy2, Fy, dx2 * Fx));
 *       trilinear acc = fmaf(wc, v, acc) over the eight corners, x fastest, from acc = +0,
 *       with wc = (wx * wy) * wz; texels outside the level are zero (zero border); level 0,
 *       and every level of an aniso = 0 grid, use the one volume (v = its texel).
 *    4. If fr > 0 and l0 < L:  s1 = the same of level l0 + 1;
 *       s = fmaf(fr, s1, (1.0f - fr) * s)
 *    5. a = fmaf(1.0f - a, s, a);  t = t + VCT_STEP_SCALE * D;  one cone step counted.
 *  The rgb channels never enter a, so this is A.6's march reduced to one channel plus the
 *  t >= t_lim end: a cone that is never limited (a directional light) takes exactly the
 *  steps of the A.6 cone with the same o, d and tau, and ends with its alpha, bit for bit.
 *  Visibility:  V = fmaxf(1.0f - a / VCT_ALPHA_STOP, 0.0f), one correctly rounded divide.
 *  A cone that saturates (a >= VCT_ALPHA_STOP) is fully dark; a cone that meets nothing
 *  (a = +0) gives exactly 1.
 *  The start (o = q = P' + N, t = 1) is K4's, and so is its known weakness: on a coarse
 *  grid a cone that leaves its surface at a grazing angle samples the surface's own voxels
 *  in its first steps and darkens itself.  No other offset is introduced here.
 *  The vis plane: vis[j][y][x] = V for a pair that is not skipped; +0 for a skipped pair
 *  and for a background pixel (pos.w == 0).
 *  Composite: contrib_c = (((A_c * color_c) * ndl) * f) * vis[j][px], summed over the
 *  lights not skipped in list order and finished as "local lights"
 *  (final = (direct + A * D) + S).  With every tan_half 0 it is vct_composite_lights_device
 *  bit for bit. */

/* ---- emissive surfaces (vct_voxelize_emission* / vct_inject_emission /
 *      vct_composite_emissive_device, include/vct_emission.h) ------------------------------
 * The emission grid reuses VCT_FIXED_ONE and VCT_KD_LIMIT and adds no literal of its own.
 *  Ke_c(t) = component c of material_ke4[material of t] (tri_material NULL: material 0).
 *  count(v) = K1's hit count of voxel v in the CURRENT voxelization (the grid the emission
 *  grid is built on).
 *      fix_c(t) = (int64)roundf(Ke_c(t) * VCT_FIXED_ONE)
 *      S_c(v)   = sum of fix_c(t) over the triangles t of THIS call whose SAT covers v
 *      E_c(v)   = (float)((double)S_c(v) / ((double)count(v) * VCT_FIXED_ONE_D))   for count(v) > 0
 *      v is emissive iff count(v) > 0 and some S_c(v) != 0.
 *    "covers" is K1's test, unchanged: the same q = (p - g0) * inv_h per vertex, the candidate
 *    range of the "K1 input rule", the same 13-axis test, touching counts.  The sums are
 *    integers, so they do not depend on the order of the triangles.
 *  A hit in a voxel with count(v) == 0 (emitter geometry that is not part of the voxelized
 *    mesh) is dropped: the emissive voxels are a subset of the occupied ones.  When the
 *    emitters are the voxelized mesh, or a subset of its triangles, E(v) is the average of Ke
 *    over ALL triangles touching v, as the albedo is the average of Kd.
 *  A triangle whose three fix_c are 0 adds nothing and has no candidates.
 *  Input rule.  Vertices: the K1 input rule (any finite vertex is legal; a triangle with a
 *    non-finite component of q is skipped, and is not an error).  Ke.r, .g, .b of every material
 *    a triangle uses must be finite, have a clear sign bit (-0.0f is refused, as the K2 input
 *    rule refuses it for a colour) and be < VCT_KD_LIMIT; otherwise, and for an index out of
 *    range or a NULL material_ke4, the call is an error (VCT_EINVAL) and the emission grid is
 *    empty afterwards.  Ke.a is not read.  With Ke >= 0, fix < 2^31 and a 32-bit count, S
 *    cannot overflow 64 bits, and E_c <= max Ke_c < 2^15.
 *  Lifetime: every vct_voxelize* and vct_load_grid empties the emission grid; vct_save_grid
 *    does not store it.
 *  vct_inject_emission(scale): at every emissive voxel, per colour channel,
 *      L_c = L_c + (scale * E_c)                  (one multiply, then one add; no fma)
 *    on the level-0 texel of the voxel; alpha and every other voxel are untouched.
 *    scale must be finite, have a clear sign bit and be <= VCT_EMISSION_SCALE_LIMIT.  The
 *    limit keeps level 0 finite: E < VCT_KD_LIMIT = 2^15, so scale * E < 2^111 * 2^15 = 2^126;
 *    K2's sum is below 2^127 ("K2 input rule", colour); their sum is below
 *    2^127 + 2^126 = 1.5 * 2^127 < FLT_MAX = (2 - 2^-23) * 2^127.
 *      VCT_EMISSION_SCALE_LIMIT = 2^126 / VCT_KD_LIMIT = 2^111.
 *  vct_composite_emissive_device: the receiver, the lights and V are those of "shadow cones"
 *    (vis given) or "local lights" (vis NULL: the walk); then
 *      p_c = (P_c - g0_c) * inv_h                 (the pixel's position, no normal offset)
 *      Em  = E(v) with v_c = (int)floorf(p_c) if 0 <= p_c < (float)n holds in float32 for all
 *            three axes (a NaN fails it) and v is emissive; else +0 in every channel
 *      final_c = ((direct_c + A_c * D_c) + S_c) + scale * Em_c      (the product, then one add)
 *    Background pixels get the clear colour as in every composite.  With an empty emission
 *    grid or scale = +0 the term is left out, so the result is the other composites' bit for
 *    bit. */
#define VCT_EMISSION_SCALE_LIMIT 2.59614843e33f  /* 2^111 exactly */

/* ---- sky light (vct_sky_cones_device / vct_inject_sky, include/vct_sky.h; no new
 *      literals) ----------------------------------------------------------------------------
 * A sky is (up, zenith, horizon, ground): a direction and three colours.
 *  Input rule.  up: the "K2 input rule" for a direction -- len = sqrtf((ux*ux + uy*uy) + uz*uz)
 *    in float32 must be finite and > 0 -- and up_n = up / len per component, as
 *    vct_inject_directional normalises its direction.  Every component of zenith, horizon and
 *    ground must be finite, have a clear sign bit (-0.0f is refused) and be <= VCT_COLOR_LIMIT
 *    (the "K2 input rule" for a colour).  Anything else is VCT_EINVAL, with nothing written and
 *    no state changed.  With |A| < VCT_KD_LIMIT = 2^15 and sum w_k T_k <= ~1 the term
 *    A * Sk that vct_inject_sky adds stays below 2^15 * 2^105 * ~3 < 2^122, so level 0 stays
 *    finite (K2's own sum is below 2^127, and below 2^121 for one light).
 *  Sky(d), for any direction d; branch-free, no fused operation, dot3 of "local lights":
 *      u     = dot3(d, up_n)
 *      s_up  = fminf(fmaxf(u, 0.0f), 1.0f)
 *      s_dn  = fminf(fmaxf(-u, 0.0f), 1.0f)
 *      Sky_c = (horizon_c + (zenith_c - horizon_c) * s_up) + (ground_c - horizon_c) * s_dn
 *    d = up_n gives the zenith colour, d = -up_n the ground colour, d perpendicular to up the
 *    horizon colour; a NaN u gives the horizon colour, since fmaxf(NaN, 0) is 0.
 *  Receiver: a G-buffer record (P, N) with P.w != 0 -- a pixel of a frame, or a bounce source
 *    of "light bounces" with its record P_c = g0_c + ((float)x_c + 0.5f) * hh.  The origin o
 *    and the cone directions d_k are exactly K4's (A.5):
 *      o_c = (P_c - g0_c) * inv_h + N_c
 *      sgn = copysignf(1.0f, N.z);  ka = -1.0f / (sgn + N.z);  kb = (N.x * N.y) * ka
 *      T = (1.0f + ((sgn * N.x) * N.x) * ka,  sgn * kb,  -(sgn * N.x))
 *      B = (kb,  sgn + (N.y * N.y) * ka,  -N.y)
 *      d_k,c = (cn_k * N_c + ct_k * T_c) + cb_k * B_c
 *    over the rows (cn, ct, cb, w) of the context's diffuse cone set: n_diffuse in {1, 9, 16}
 *    (VCT_CONES1 / 9 / 16), aperture tau = VCT_TAN30 for 1 and 9 cones, VCT_TAN20 for 16.
 *  Per cone k, in set order:
 *      a_k = the result of steps 1-5 of "shadow cones" with o, d = d_k, tau and t_lim = +inf
 *    (so the "light is reached" end never applies).  This is the alpha of K4's own diffuse
 *    cone k, bit for bit, and the cone takes K4's steps: a sky call counts exactly the cone
 *    steps of K4's diffuse cones on the same records.
 *      T_k = fmaxf(1.0f - a_k / VCT_ALPHA_STOP, 0.0f)        (one correctly rounded divide)
 *  Per receiver, from acc = vis = +0, in set order:
 *      acc_c = fmaf(w_k * T_k, Sky_c(d_k), acc_c)            (the product w_k * T_k rounded first)
 *      vis   = fmaf(w_k, T_k, vis)
 *    Sk = (acc.rgb, vis).  A background record (P.w == 0), and every record of a context with
 *    n_diffuse = 0, gives +0 in all four channels.
 *  A non-finite o or d_k (a non-finite position or normal) makes p = o + d t fail the inside
 *    test of step 1 before the first sample: a_k = +0, T_k = 1, and Sky(d_k) is the horizon
 *    colour where u is NaN.  No sample is ever taken at a non-finite p.
 *  The start (o = P' + N, t = 1) is K4's, and K4's self-occlusion on coarse grids comes with
 *    it ("shadow cones" says the same of its start): a cone that leaves its surface at a
 *    grazing angle samples the surface's own voxels in its first steps, so on the Cornell
 *    box at 16^3 and 32^3 about half of the cones saturate and almost none ends with T
 *    exactly 1.  No other offset is introduced here.
 *  vct_sky_cones_device: sky4[px] = Sk; with diffuse4_inout, at every valid pixel
 *      diffuse_c = diffuse_c + Sk_c                          (one add per channel, c = r, g, b)
 *    and alpha, and every background pixel, untouched.  A diffuse component that is -0.0f
 *    becomes +0.0f when Sk_c is +0 (an all-zero sky changes no other bit).
 *  vct_inject_sky: at every bounce source v ("light bounces": occupied, nonzero normal), on
 *    the level-0 texel of v,
 *      L_c = L_c + A_c(v) * Sk_c(v)                          (one multiply, then one add; no fma)
 *    alpha untouched, every other voxel untouched; then the pyramid is rebuilt from that level
 *    0.  Level 0 stays nonzero exactly at the occupied voxels and every alpha of the pyramid
 *    is unchanged, so a_k, T_k and vis are the same before and after. */

/* ---- dynamic layer (vct_voxelize_dynamic*, include/vct_dynamic.h; no new arithmetic) ----
 *  The context holds at most one dynamic layer: a set of triangles on top of the static
 *    grid, the grid of the last successful vct_voxelize* (or vct_load_grid).  Let S be the
 *    static mesh and D the layer's.  union(S, D) is the mesh of S's vertices followed by D's,
 *    S's triangles followed by D's (D's vertex indices offset by S's vertex count), S's
 *    materials followed by D's (D's material ids offset by S's material count).
 *  Equality: after vct_voxelize_dynamic*(D) the context is, bit for bit, the context after
 *    vct_voxelize(union(S, D)): K1's sums and counts, albedo / occupancy and normals, the
 *    occupancy bits, the set of occupied voxels, and therefore everything computed from them
 *    (level 0 of every vct_inject_*, every mip face, K4, the shadow and sky marches, the
 *    bounce sources, every composite), and both G-buffer passes (S's triangles then D's, in
 *    that index order: ties go to the lower index).  This holds after any sequence of
 *    updates, because S_union(v) = S_S(v) + S_D(v) and count_union(v) = count_S(v) +
 *    count_D(v) are sums of integers: an update subtracts the previous layer's terms and adds
 *    the new layer's, modulo 2^64, exactly.  n_idx == 0 removes the layer: the grid is S's.
 *  A voxel only the removed layer occupied: an all-zero record, albedo = normal = (0,0,0,0),
 *    a +0 level-0 texel, a clear occupancy bit, absent from the occupied list.  Records are
 *    zero everywhere outside the occupancy.
 *  Input rule: K1's ("K1 input rule"): a finite vertex anywhere is legal; a triangle with a
 *    non-finite voxel-unit vertex is skipped (no candidates, a zero triangle for the G-buffer
 *    passes); Kd must be finite with |Kd| < VCT_KD_LIMIT.  The layer takes Kd materials only.
 *  Packed sums: while the grid's records are packed ("K1", two sums per word), a voxel the
 *    update touched must keep count x max|value| < 2^31 with max|value| the larger of the
 *    static pass's and the layer's; otherwise the occupied records are converted in place to
 *    one sum per word and the layer is added in that form.  The sums, and so every result,
 *    are the same either way.
 *  State: a new vct_voxelize* or vct_load_grid drops the layer record; what it leaves is the
 *    static grid.  vct_save_grid with a layer in place saves the union as a plain grid.
 *  The call invalidates what a voxelization invalidates: level 0, the mips, bounces,
 *    emission and sky marks, the emission grid and the bounce source list; vct_inject_*
 *    and vct_build_mips (a full build) follow it as they follow vct_voxelize. */

/* ---- dynamic objects (vct_objects_define / vct_objects_update*, include/vct_objects.h;
 *      tests/objects_ref.py restates the transform rule, the feature's only new arithmetic) ----
 *  The context holds at most one object set: n_objects rigid meshes O_0, O_1, ... in object
 *    space, registered once, each with a pose P_k = (m[16], visible); every object starts
 *    hidden.  The set sits on top of the static grid as the dynamic layer does, and excludes it.
 *  The transform rule: T(O, P) is O with every vertex (x, y, z) replaced by
 *        x' = ((m[0] x + m[4] y) + m[8]  z) + m[12]
 *        y' = ((m[1] x + m[5] y) + m[9]  z) + m[13]
 *        z' = ((m[2] x + m[6] y) + m[10] z) + m[14]
 *    in float32, one rounding per operation, no fma contraction; m is column-major and m[3],
 *    m[7], m[11], m[15] are not read.  Any matrix is legal: its contents are data, never a
 *    status.  A non-finite result makes the triangle a skipped one under the K1 input rule.
 *    Nothing is special-cased, so an identity matrix maps -0.0f to +0.0f (-0 + 0 = +0), and an
 *    infinite coordinate stays in its own row and makes the vertex's other two coordinates NaN
 *    (0 x inf).  T of a hidden object (visible == 0) is its
 *    triangles with every vertex NaN: skipped by K1, zero triangles for the G-buffer passes.
 *  Equality: let S be the static mesh and P_k the last pose given for object k.  After any
 *    sequence of vct_objects_define / vct_objects_update* calls the context is, bit for bit,
 *    the context after vct_voxelize(union(S, T(O_0, P_0), T(O_1, P_1), ...)), union being the
 *    dynamic layer's concatenation extended to several meshes, in definition order, the set's
 *    one material table behind S's.  Everything the layer's equality clause lists holds: K1's
 *    sums and counts, albedo / occupancy and normals, the occupancy bits and the occupied set,
 *    level 0 of every vct_inject_*, every mip face, K4, the marches, the bounce sources, every
 *    composite, and both G-buffer passes in that triangle order.  It holds because an update
 *    subtracts, modulo 2^64, exactly the terms the named objects' previous poses added, and
 *    adds the new poses' terms; every other object's terms stay.  After vct_objects_define
 *    the grid is S's; n_objects == 0 removes the set, and the grid is S's again.
 *  A voxel only a moved or hidden object occupied: an all-zero record, albedo = normal =
 *    (0,0,0,0), a +0 level-0 texel, a clear occupancy bit, absent from the occupied list.
 *  Materials: Kd only, one table for the set, under the K1 input rule; the set's triangles
 *    shade flat and are opaque.  A live shading set and cutout table describe S's triangles and
 *    are carried over every update.
 *  Packed sums: the layer's rule, with max|value| the larger of the static pass's and the
 *    running maximum over everything the set ever added (conservative; the sums are the same
 *    either way).  When the conversion is needed after a subset moved, what that update added
 *    is retracted, the occupied records are converted, and the same terms are added again in
 *    the one-sum-per-word form.
 *  State: before a successful vct_voxelize* / vct_load_grid every call is VCT_ESTATE.  A new
 *    vct_voxelize* / vct_load_grid drops the set; what it leaves is the static grid, and an
 *    update is VCT_ESTATE until the set is defined again.  vct_objects_define with a layer in
 *    place and vct_voxelize_dynamic* with a set defined are VCT_ESTATE; either is removed by its
 *    own empty call.  vct_save_grid with a set saves the union as a plain grid.
 *  Errors are found on the host before any launch (include/vct_objects.h lists them): the
 *    context, the set and the marks stay exactly as they were.
 *  An update of n > 0 objects invalidates what vct_voxelize_dynamic invalidates; n == 0
 *    touches nothing. */

/* ---- mixed-resolution trace (include/vct_mixed.h; tests/mixed_ref.py restates it) ----
 *  All arithmetic is float32, one rounding per operation, no fma contraction; integers are
 *    exact.  K4 is a function of a pixel's G-buffer record (ray order and tile layout change
 *    no bit), so tracing a frame of copied records gives the copied pixels' own values.
 *  Cone selection (vct_trace_cones_device): K4 with n_diffuse = 0 for VCT_CONES_SPECULAR, with
 *    specular = 0 for VCT_CONES_DIFFUSE.  The selected plane and the step and texel counts of
 *    the selected cones are those of the full launch; a cone set the context lacks gives +0.
 *  Frames: factor f in {2, 4}; low frame wl = ceil(w / f) by hl = ceil(h / f); low pixel (X, Y)
 *    covers the full pixels x in [f X, f X + f), y in [f Y, f Y + f), clipped to the frame.
 *  Pick: candidates are the block's valid pixels (pos.w != 0, K4's rule).  With d = pos - eye,
 *      key = ((dx dx + dy dy) + dz dz),   a NaN key counts as +Inf;
 *    the smallest key wins, a tie goes to the lower row-major index y w + x (nearest surface:
 *    a silhouette belongs to the foreground).  The three records are copied bit for bit,
 *    lo_src[Y][X] = y w + x.  No candidate: +0 records and lo_src = 0xffffffff.
 *  Upsample of pixel p = (x, y) with records P, N over any low plane V:
 *    background (P.w == 0): +0 in all four channels.
 *    representative (lo_src[y / f][x / f] == y w + x): V[y / f][x / f], all four channels, exactly.
 *    otherwise four bilinear taps, in integers, in x and likewise in y:
 *      t = 2 x + 1 - f,  X0 = floor(t / 2f) (X0 may be -1),  r = t - 2f X0,
 *      tap X0 weighs 2f - r, tap X0 + 1 weighs r;  bw = (x weight) (y weight) <= 64.
 *    Taps are visited in the order (0,0), (1,0), (0,1), (1,1).  A tap is dropped when it lies
 *    outside the low frame, bw = 0, or its lo_src = 0xffffffff.  A remaining tap q (records
 *    Pq, Nq) is accepted when both
 *      c = (Nx Nqx + Ny Nqy) + Nz Nqz >= normal_cos
 *      d = |(Nx (Pqx - Px) + Ny (Pqy - Py)) + Nz (Pqz - Pz)| <= plane_eps
 *    hold; a NaN fails either test.  Per channel the result is S / W: S = bw V of the first
 *    accepted tap, then S = S + bw V for each further one (bw converted to float, one multiply,
 *    one add); W = float(integer sum of the accepted bw); one correctly rounded division.
 *    W = 0: the pixel is a hole.
 *  Holes: hole k is the k-th hole in row-major pixel order.  k < max_holes: the pixel's three
 *    records go to entry k of the packed hole G-buffer (64 pixels wide, ceil(max_holes / 64)
 *    rows; every entry from min(count, max_holes) on is +0), hole_px[k] = y w + x, and the
 *    plane value is left for the scatter.  k >= max_holes (overflow): the fallback value, the
 *    same S / W over every remaining tap without the two tests; the pixel's own block always
 *    supplies one.  count = the number of holes; stats = {representatives, interpolated,
 *    holes, overflowed} over valid pixels.
 *  Scatter: plane[hole_px[k]] = hole_plane[k] for k < min(count, max_holes).
 *  Frame (vct_trace_mixed_device): pick; K4's diffuse cones over the low frame; upsample into
 *    the diffuse plane; K4's diffuse cones over the hole frame; scatter; K4's specular cone at
 *    full resolution.  Every representative and every listed hole therefore carries the
 *    full-resolution trace's diffuse value bit for bit, and the specular plane is the
 *    full-resolution trace's.  cone_steps = the diffuse steps of the representatives and the
 *    listed holes plus every specular step.
 *  Input rule: normal_cos finite in [-1, 1]; plane_eps finite, >= 0, sign bit clear;
 *    max_holes >= 1 (0 means ceil(w h / 8)); anything else is VCT_EINVAL with nothing written. */

/* ---- volumetric fog (include/vct_fog.h; tests/fog_ref.py restates it) -------------------
 *  All arithmetic is float32, one rounding per operation, no contraction; the fused
 *    operations are the fmaf() written below.  dot3 is "local lights"'.
 *  Medium: (density, albedo, ambient, level, step), the input rule of vct_fog.h:
 *    density finite, sign bit clear, <= VCT_FOG_DENSITY_LIMIT; albedo_c finite, in [0, 1], sign
 *    bit clear; ambient finite and >= 0; 1 <= level and m = n >> level >= 4; 0.25 <= step <= 4.
 *      sigma_v = (density * E) / (float)n        (multiply, then divide; must be finite)
 *      cs = 2^level,  ds = step * cs             (both exact)
 *  Scatter volume (vct_build_fog): cell (i, j, k), 0 <= i, j, k < m, has the centre
 *      x_c = ((float)i + 0.5f) * cs              (exact), likewise y_c, z_c, in voxel units.
 *    Per light j in list order, with the per-light host constants of "local lights":
 *      directional:  l = the light's l, att = 1.0f, t_lim = +inf; never skipped
 *      point, spot:  d = pL - x_c, r2 = dot3(d, d); skipped unless r2 > 0
 *                    r = sqrtf(r2), l_c = d_c / r, t_lim = r
 *                    u = r2 * inv_rr, w = fmaxf(1.0f - u, 0.0f), att = (w * w) / (1.0f + r2 * h2)
 *      spot only:    cd = dot3(l, a), s = fminf(fmaxf((cd - cos_outer) * inv_span, 0.0f), 1.0f)
 *                    att = att * (s * s)
 *      skipped unless att > 0 (out of range, outside the cone).  This is "local lights"' f
 *      with the receiver q = x_c and without the n.l cosine: a medium has no normal.
 *      tau = fminf(fmaxf(tan_half[j], VCT_SPEC_TAU_MIN), VCT_SPEC_TAU_MAX)
 *      a_j = steps 1-5 of "shadow cones" with o = x_c (no normal offset), d = l, tau, t_lim
 *      V_j = fmaxf(1.0f - a_j / VCT_ALPHA_STOP, 0.0f)
 *      acc_c = fmaf(C_j,c, att * V_j, acc_c)     from acc = +0 (the product att * V_j rounded first)
 *    A skipped light marches no cone and leaves acc as it is.
 *    Ambient (ambient > 0 and n_diffuse > 0): I+ and I- are the rgb of K4's diffuse plane (A.5,
 *    A.6; the context's diffuse cone set, no specular cone) for the records
 *      hh = E / (float)n,  P_c = g0_c + x_c,c * hh  (multiply, then add),  P.w = 1,
 *      normal (0, +1, 0) for I+, (0, -1, 0) for I-
 *      A_c = 0.5f * (I+_c + I-_c);               A = +0 when n_diffuse = 0
 *    Cell:  ambient == 0:  S_c = albedo_c * (VCT_FOG_PHASE * acc_c)
 *           ambient > 0:   S_c = albedo_c * fmaf(ambient, A_c, VCT_FOG_PHASE * acc_c)
 *           S.w = +0.
 *  Rays (vct_fog_rays_device): o_c = (eye_c - g0_c) * inv_h, once, on the host.
 *    valid pixel (pos.w != 0): e_c = (P_c - g0_c) * inv_h, v = e - o,
 *      len = sqrtf((vx*vx + vy*vy) + vz*vz), d_c = v_c / len       (the K2 direction rule)
 *    background pixel with a camera: d = the caster's primary-ray direction of the pixel
 *      (vct_frame.hip pixel_ray: normalised by il = 1.0f / sqrtf(dot3(d, d)), d_c * il), len = +inf
 *    background pixel without a camera: (+0, +0, +0, +0)
 *    not a ray -- !(len > 0), a len of a valid pixel that is not finite, or a non-finite
 *      component of d: (+0, +0, +0, +0).
 *  March (vct_fog_march_device), per pixel, record (d, len), o as above (must be finite):
 *    null record: !(len > 0) or a non-finite d_c: result (0, 0, 0, 1), no sample.
 *    Slab, per axis c, nf = (float)n, inv = 1.0f / d_c:
 *      d_c == 0 or inv not finite (|d_c| <= 2^-128): the axis does not clip when
 *        0 <= o_c <= nf holds, and empties the segment otherwise
 *      else ta = (0.0f - o_c) * inv, tb = (nf - o_c) * inv, tn_c = fminf(ta, tb), tf_c = fmaxf(ta, tb)
 *      t0 = fmaxf(fmaxf(fmaxf(0.0f, tn_x), tn_y), tn_z)   over the clipping axes
 *      t1 = fminf(fminf(fminf(len, tf_x), tf_y), tf_z)
 *      the segment is empty unless t1 > t0.  o and inv are finite and inv != 0, so no t is
 *      ever NaN (the discipline of the K2 walk's "NaN step" rule).
 *    Samples: span = t1 - t0, N = (int)fminf(ceilf(span / ds), (float)VCT_FOG_MAX_STEPS)
 *      sample i < N:  ts = t0 + ((float)i + 0.5f) * ds,  p_c = o_c + d_c * ts  (multiply, add)
 *      its length:  ds for i < N - 1;  fminf(span - (float)(N - 1) * ds, ds) for i = N - 1
 *      a_i = fminf(sigma_v * length, 1.0f)
 *    Trilinear S(p) (A.5's shape, edge clamp instead of zero border): c = p * 2^-level - 0.5f
 *      (the product exact), fl = floorf(c), w = c - fl, weights (1.0f - w, w) per axis, corner
 *      indices (int)fl and (int)fl + 1 each clamped to [0, m - 1];
 *      S_c = fmaf(wc, cell_c, S_c) over the eight corners, x fastest, from +0, wc = (wx * wy) * wz.
 *    Front to back from F = +0, T = 1, before each sample: end if T < VCT_FOG_T_STOP;
 *      F_c = fmaf(T * a_i, S_c, F_c);  T = T * (1.0f - a_i);  one sample counted.
 *    The per-step opacity is linear in the length on purpose: no transcendental enters.
 *  Apply (vct_fog_apply_device): rgb_c = fmaf(rgb_c, T, F_c), alpha untouched.  The RGBA8
 *    frame, alpha 255, with tone(v) = (max(v / (1 + v), 0))^VCT_INV_GAMMA and q(v) = the
 *    composite's rounding to 8 bits: a pixel whose incoming alpha is not 0 gets q(tone(rgb_c)) of
 *    the new rgb, the composite's own present step.  A pixel with alpha 0 is a background pixel of
 *    a composite, which presents its clear colour as it is, without the tone curve; the fog goes
 *    over it in display space, q(fmaf(rgb_c, T, tone(F_c))) with the incoming rgb, so that
 *    T = 1, F = 0 reproduces the composite's byte.  Without a linear frame the incoming pixel is
 *    (0, 0, 0, 0): the fog layer alone, q(tone(F_c)). */
#define VCT_FOG_PHASE          0.0795774715f  /* 1 / (4 pi)                                  */
#define VCT_FOG_T_STOP         0.00390625f    /* 2^-8                                        */
#define VCT_FOG_MAX_STEPS      4096           /* > 1024 sqrt(3) / (0.25 * 2): the diagonal of
                                                 1024^3 at level 1, step 0.25 (3548 samples) */
#define VCT_FOG_DENSITY_LIMIT  1048576.0f     /* 2^20 per world unit                         */

/* ---- temporal accumulation (include/vct_temporal.h; tests/temporal_ref.py restates it) ----
 *  All arithmetic is float32, one rounding per operation, no contraction; integers are exact.
 *    dot3 is "local lights"'.  Per pixel (x, y) of a w x h frame with records P, N, the planes'
 *    values cur_p (p < n_planes), and, with a history, last frame's camera (eye', front', right',
 *    up', tan_half, aspect: the host constants of vct_view.h camera_fields for this w and h,
 *    tan_half = tanf(zoom_deg * 0.5f * 3.14159265358979f / 180.0f), aspect = (float)w / (float)h),
 *    last frame's records Pq, Nq, planes hist_p and lengths hist_len.
 *  Background (P.w == 0): +0 in every channel of every out_p, out_len = 0; not counted.
 *  Reset: out_p = cur_p bit for bit in every plane, out_len = 1.  A valid pixel is counted in
 *    exactly one of reused, reset_offscreen and reset_rejected; valid is their sum.
 *    reset_offscreen: no history (prev_cam == NULL); motion4.w == 0; a failed projection test.
 *    reset_rejected: no accepted tap (W = 0); a non-finite blended history; k = 1 (max_len = 1).
 *  Previous position: q = motion4.xyz, or P.xyz when motion4 is NULL (a NaN motion4.w is not 0).
 *  Projection (the inverse of vct_view.h pixel_ray):
 *      v_c = q_c - eye'_c,  z = dot3(v, front'),  a = dot3(v, right'),  b = dot3(v, up')
 *    reset unless z > 0;
 *      kx = tan_half * aspect,  sx = a / (z * kx),  sy = b / (z * tan_half)
 *      fx = ((sx + 1.0f) * 0.5f) * (float)w - 0.5f,  fy = ((1.0f - sy) * 0.5f) * (float)h - 0.5f
 *    reset unless -1.0f < fx < (float)w and -1.0f < fy < (float)h.  A NaN fails every comparison;
 *    the comparisons also make the integer conversions below safe.
 *  Taps, in integers, in x and likewise in y:
 *      X16 = (int)floorf(fx * 16.0f + 0.5f),  x0 = X16 >> 4 (floor: -1 .. w),  rx = X16 & 15,
 *      tap x0 weighs 16 - rx, tap x0 + 1 weighs rx;  bw = (x weight) (y weight), summing to 256.
 *    Taps are visited in the order (0,0), (1,0), (0,1), (1,1).  A tap is dropped when it lies
 *    outside the frame, bw = 0, its Pq.w == 0, or its hist_len == 0.  A remaining tap is
 *    accepted when both
 *      c = dot3(N, Nq) >= normal_cos
 *      d = |dot3(N, Pq - q)| <= plane_eps        (Pq - q per component, then the dot3)
 *    hold; a NaN fails either test.
 *  Blended history, per plane and channel, by the upsample's rule: S = bw hist of the first
 *    accepted tap, then S = S + bw hist for each further one (bw converted to float, one
 *    multiply, one add); W = float(integer sum of the accepted bw); H = S / W, one correctly
 *    rounded division.  W = 0 is a reset.  If any of the 4 n_planes values of H is not finite the
 *    pixel resets, so one bad sample cannot poison a pixel for ever.
 *  Blend: L = min of hist_len over the accepted taps (>= 1), k = min(L, max_len - 1) + 1, which
 *    is min(L + 1, max_len) without the overflow.  k = 1: a reset (H + (cur - H) * 1 is not cur
 *    in floats).  Otherwise wk = 1.0f / (float)k and
 *      out = H + (cur - H) * wk                  (subtract, multiply, add)
 *    out_len = k, and the pixel counts as reused.
 *  A single tap of bw = 256 gives H = hist exactly (256 hist and the division are exact unless
 *    256 hist overflows, which resets), so under an unchanged camera and G-buffer a constant
 *    input stays that constant: H + (c - H) * wk = c + 0 (a constant -0 becomes +0).
 *  Input rule: normal_cos finite in [-1, 1]; plane_eps finite, >= 0, sign bit clear; max_len in
 *    1 .. VCT_TEMPORAL_MAX_LEN; tan_half finite and > 0, every component of eye', front',
 *    right', up' finite; anything else is VCT_EINVAL with nothing written. */

/* ---- sky in view (vct_sky_specular_device / vct_sky_background_device,
 *      include/vct_sky_view.h; no new literals; tests/sky_view_ref.py restates it) -------------
 *  All arithmetic is float32, one rounding per operation, no contraction.  The sky record, its
 *    input rule, up_n and Sky(d) are those of "sky light"; dot3 is "local lights"'.
 *  Specular sky, per valid pixel (pos.w != 0, K4's rule) with records P, N, roughness = alb.w:
 *      o_c = (P_c - g0_c) * inv_h + N_c                           (K4's origin, A.5)
 *      v_c = eye_c - P_c;  vl = sqrtf((vx*vx + vy*vy) + vz*vz);  v_c = v_c / vl
 *      ndv = dot3(N, v);  k2 = 2.0f * ndv;  r_c = k2 * N_c - v_c  (A.6's specular cone)
 *      tau = fminf(fmaxf(roughness, VCT_SPEC_TAU_MIN), VCT_SPEC_TAU_MAX)
 *      a   = the result of steps 1-5 of "shadow cones" with o, d = r, tau and t_lim = +inf
 *    (the "light is reached" end never applies).  This is the alpha of K4's own specular cone,
 *    bit for bit, and the cone takes K4's steps: a call counts exactly the cone steps of K4's
 *    specular cones on the same frame.
 *      T   = fmaxf(1.0f - a / VCT_ALPHA_STOP, 0.0f)               (one correctly rounded divide)
 *      S_c = T * Sky_c(r)                                         (one multiply per channel)
 *    skyspec4[px] = (S.rgb, T).  A background pixel (pos.w == 0), and every pixel of a context
 *    with specular = 0, gives +0 in all four channels and counts no step.
 *    With spec4_inout, at every valid pixel
 *      spec_c = spec_c + S_c                                      (one add per channel, c = r, g, b)
 *    and alpha, and every background pixel, untouched.  A specular component that is -0.0f
 *    becomes +0.0f when S_c is +0 (an all-zero sky changes no other bit).
 *  Hostile records are legal.  A non-finite r -- a non-finite position or normal, an eye whose
 *    v.v overflows, or an eye on the pixel itself (vl = 0, v = 0 / 0) -- makes p = o + r t
 *    fail the inside test of step 1 before the first sample: a = +0, T = 1, no step, and Sky(r)
 *    is the horizon colour where u is NaN (fmaxf(NaN, 0) is 0), so S is the horizon colour.  A
 *    NaN roughness clamps to VCT_SPEC_TAU_MIN (fmaxf(NaN, x) is x).  No sample is ever taken
 *    at a non-finite p.
 *  Sky background, per pixel with pos.w == 0 (-0.0f is background) of a w x h frame:
 *      d   = the caster's primary-ray direction of the pixel (vct_view.h pixel_ray with the host
 *            constants of camera_fields: tan_half = tanf(zoom_deg * 0.5f * 3.14159265358979f /
 *            180.0f), aspect = (float)w / (float)h; normalised by il = 1.0f / sqrtf(dot3(d, d)),
 *            d_c * il), as "volumetric fog" reads it for its background rays
 *      c   = Sky(d)
 *      linear4[px] = (c.r, c.g, c.b, 1.0f)
 *      rgba8[px]   = q(tone(c.r)) | q(tone(c.g)) << 8 | q(tone(c.b)) << 16 | 255 << 24
 *    with tone and q the composite's present step ("volumetric fog", apply).  Alpha 1 marks the
 *    pixel as shaded: vct_fog_apply_device then takes it through the tone curve, not as a
 *    clear-colour pixel.  Valid pixels are not read beyond pos.w and not written. */

/* ---- cone queries (vct_cone_query_device, include/vct_query.h; tests/query_ref.py restates
 *      it) ------------------------------------------------------------------------------------
 *  All arithmetic is float32, one rounding per operation, no contraction; the fused operations
 *    are the fmaf() calls named here.  A cone is the record (p, tau, d, t_lim, off, valid).
 *  valid == 0 (-0.0f too): out4 = +0 in all four channels, steps = 0; nothing is marched.  A
 *    NaN valid is not 0.
 *  Origin, per component:  o_c = ((p_c - g0_c) * inv_h) + off_c   (K4's origin, A.5, with off in
 *    the place of the normal).
 *  Direction: d as given, never normalised.  Faces f_c from d_c >= 0.0f (a NaN or -0 component
 *    selects the negative face, as in K4), face weights wd_c = d_c * d_c.
 *  Aperture: tau' = fminf(fmaxf(tau, VCT_SPEC_TAU_MIN), VCT_SPEC_TAU_MAX) (a NaN tau clamps to
 *    VCT_SPEC_TAU_MIN), tau2 = 2.0f * tau'.
 *  March (A.6, K4's): c = (0, 0, 0), a = 0, t = 1.0f, steps = 0; repeat at most
 *    VCT_QUERY_MAX_STEPS times:
 *      1. stop unless a < VCT_ALPHA_STOP;  stop unless t <= t_max = (float)n * VCT_SQRT3;
 *         stop if t >= t_lim (false for a NaN t_lim, which therefore never limits; t_lim <= 1
 *         gives zero steps);  q_c = o_c + d_c * t;  stop unless 0 <= q_c <= (float)n for every c
 *         (a NaN fails)
 *      2. D = fmaxf(1.0f, tau2 * t);  m = fminf(log2(D), (float)L) with the log2 above;
 *         l0 = (int)m;  fr = m - (float)l0
 *      3. s = S_l0(q);  if fr > 0 and l0 < L:  s1 = S_(l0+1)(q) and per channel
 *         s = fmaf(fr, s1, (1.0f - fr) * s)
 *      4. oma = 1.0f - a;  c = fmaf(oma, s.rgb, c);  a = fmaf(oma, s.a, a)   (a from the old oma)
 *      5. t = t + VCT_STEP_SCALE * D;  steps += 1
 *    The level sample S_l(q), four channels: u_c = q_c * 2^-l - 0.5f, i_c = floorf(u_c),
 *    w1_c = u_c - i_c, w0_c = 1.0f - w1_c; the eight corner texels i + (dx, dy, dz) in the order
 *    dz, dy, dx (dx fastest), each with wc = (wx * wy) * wz; a corner outside the level adds
 *    nothing; per channel acc = fmaf(wc, v, acc) from acc = +0, where v is the texel (level 0,
 *    or an isotropic pyramid) or, on an anisotropic level l > 0,
 *      v = fmaf(wd_z, T_fz, fmaf(wd_y, T_fy, wd_x * T_fx))
 *    of the corner's texels in the three selected faces.
 *    t grows by at least 0.5 a step, so a cone takes fewer than 2 n sqrt(3) + 1 steps; the
 *    integer cap is above that for n <= 1024 and is never reached by legal arithmetic.  It
 *    bounds the loop in the kernel and in the reference alike.
 *  out4 = (c.rgb, a): the layout of K4's spec4.  No sample is ever taken at a non-finite q.
 *  Identities (bit for bit): p = P, off = N, d = "sky in view"'s r, tau = alb.w, t_lim = +inf is
 *    the pixel's spec4, with the steps of K4's specular cone; the rows (cn, ct, cb, w) of the
 *    context's diffuse set with d_k = (cn * N + ct * T) + cb * B, tau = VCT_TAN30 (VCT_TAN20 for
 *    16), accumulated in row order as irr = fmaf(w, c_k, irr), occ = fmaf(w, a_k, occ), are
 *    diffuse4 = (irr, 1.0f - occ). */

/* ---- probe grid (vct_probe_build_device / vct_probe_sample_device, include/vct_query.h) ------
 *  Input rule: origin finite, spacing finite and > 0, each dim in 1 .. VCT_PROBE_MAX_DIM (256,
 *    include/vct_query.h).
 *  Build.  Probe (i, j, k), stored at [k][j][i], stands at P_c = fmaf((float)i_c, spacing,
 *    origin_c).  Face f (VCT_FACE_* order) = the out4 of the cone query p = P, off = +0,
 *    d = the unit axis of f (the other two components +0), tau = VCT_SPEC_TAU_MAX,
 *    t_lim = +inf, valid = 1.  With o the cone's origin (above; the same for the six faces),
 *    state = 1 when 0 <= o_c < (float)n for every c and K1's occupancy of the voxel
 *    floorf(o) is 0; otherwise (a wall, outside the grid, an overflowed P) state = 0.
 *  Sample, per point with pos.w != 0, per axis c with D_c = dims_c:
 *      g = (P_c - origin_c) / spacing                     (one correctly rounded division)
 *      g = fminf(fmaxf(g, 0.0f), (float)(D_c - 1))        (a NaN becomes 0)
 *      i0 = D_c == 1 ? 0 : min((int)floorf(g), D_c - 2);  fr = g - (float)i0
 *      w_c[0] = 1.0f - fr,  w_c[1] = fr
 *    The eight corners in the order cn = dx + 2 dy + 4 dz, wc = (wx[dx] * wy[dy]) * wz[dz].  A
 *    corner with i0 + d >= D_c on some axis (only when D_c == 1), or whose state is 0, is left
 *    out.  Over the kept corners, in order: W = W + wc from +0, and for each of the three
 *    faces the normal selects (f_c from n_c >= 0.0f, as a cone's) and each channel
 *      S_f = fmaf(wc, probe[f], S_f)                      from +0
 *    Then with wn_c = n_c * n_c (the normal as given)
 *      V = fmaf(wn_z, S_fz, fmaf(wn_y, S_fy, wn_x * S_fx))       per channel
 *    W > 0:  out4 = (V.r / W, V.g / W, V.b / W, 1.0f - V.a / W);  otherwise (W = 0, or a NaN)
 *    out4 = (+0, +0, +0, 1.0f) and the point is a miss.  A background point (pos.w == 0, -0 too)
 *    gets +0 in all four channels and is no miss. */

/* ---- voxel view (vct_voxel_pick_device / vct_voxel_view_device, include/vct_voxview.h;
 *      tests/voxview_ref.py restates it) ---------------------------------------------------------
 *  All arithmetic is float32, one rounding per operation, no contraction; the fused operations
 *    are the fmaf() calls named here.  A ray is (org, v, t_lim); the launch has a level l with
 *    n_l = n >> l cells per axis, nf = (float)n_l, and a solid source.
 *  Ray of a pick: org = org4.xyz, v = dir4.xyz, t_lim = dir4.w.  Ray of view pixel (x, y):
 *    org = cam->position, v = the d of the "G-buffer input rule" (vct_view.h pixel_ray, already
 *    normalised there, and normalised once more below like any other v), t_lim = +inf.
 *  Origin:  o_c = (org_c - g0_c) * inv_h  (the fog rays' expression; the view evaluates it once on
 *    the host),  ol_c = o_c * 2^-l  (exact).
 *  Direction (the K2 direction rule):  len = sqrtf(dot3(v, v)),  d_c = v_c / len.
 *  Limit:  lim = t_lim, or +inf when t_lim is a NaN;  ll = lim * 2^-l  (exact).
 *  Not a ray -- len not finite or not > 0, or a non-finite component of o or of d: a miss with
 *    0 steps.  (A non-finite ol has a non-finite o; !(ll > 0) is an empty segment below.)
 *  Slab: "volumetric fog"'s, per axis c with nf, ol and len = ll:  inv = 1.0f / d_c;  an axis with
 *    d_c == 0 or inv not finite does not clip when 0 <= ol_c <= nf and empties the segment
 *    otherwise; else ta = (0.0f - ol_c) * inv, tb = (nf - ol_c) * inv, tn_c = fminf(ta, tb),
 *    tf_c = fmaxf(ta, tb);  t0 = the largest of 0 and the clipping axes' tn_c,  t1 = the smallest
 *    of ll and their tf_c;  the segment is empty unless ll > 0 and t1 > t0.  An empty segment is a
 *    miss with 0 steps.
 *    t0 also names its axis:  t0 = +0, a0 = none;  then for c = x, y, z in turn, if the axis clips
 *    and tn_c > t0:  t0 = tn_c, a0 = c.  That is the fmaxf chain's value (a zero t0 is +0 here
 *    whatever the sign of a zero tn_c), with ties going to x, then y, then z.  a0 = none exactly
 *    when t0 == 0, and then every clipping axis has tn_c <= 0 <= tf_c and every other axis holds
 *    0 <= ol_c <= nf: the origin lies in the closed grid, on its surface included.
 *    t1 > t0 makes t0 finite.
 *  Walk (A.3's, as the K2 input rule writes it), with sign / td from d:  s_c = sign(d_c),
 *    td_c = 1.0f / fabsf(d_c) (+inf where d_c == 0); an axis whose td_c is not finite does not
 *    move: s_c = 0, tm_c = +inf.  (td_c is finite exactly when the axis clips.)
 *      p_c = ol_c + d_c * t0                         (multiply, add)
 *      v_c = (int)fminf(fmaxf(floorf(p_c), 0.0f), nf - 1.0f)      (clamped before the conversion)
 *      tm_c = ((float)(v_c + 1) - p_c) * td_c  for s_c > 0,  (p_c - (float)v_c) * td_c  for s_c < 0
 *      face = 6 when a0 = none, else 2 a0 + (s_a0 > 0 ? 0 : 1);   te = t0;   steps = 0
 *    Repeat at most VCT_VOXVIEW_STEPS_PER_CELL * n_l times:
 *      1. steps += 1.  If cell v is solid: a hit, record (v_x + n_l (v_y + n_l v_z), face, steps,
 *         bits of te * 2^l); end.
 *      2. a = x if tm_x <= tm_y and tm_x <= tm_z, else y if tm_y <= tm_z, else z;
 *         tn = t0 + tm_a  (tm_a before the addition of step 4).  If tn >= ll: a miss; end.
 *      3. v_a += s_a.  If v_a < 0 or v_a >= n_l: a miss; end.
 *      4. tm_a = tm_a + td_a;  face = 2 a + (s_a > 0 ? 0 : 1);  te = tn.
 *    A miss is (0xFFFFFFFF, 7, steps, bits of +inf).  The cell is tested first, then stepped.
 *    No t is a NaN: t0 is finite; ol_c and d_c * t0 are finite (|d_c| <= 1 up to rounding), so
 *    p_c is finite or, by overflow of the sum, one infinity, never a NaN; v_c is an integer in
 *    [0, n_l - 1]; td_c of a moving axis is finite and >= 2^-1 (not 0), so tm_c is a product of a
 *    finite or infinite factor and a finite positive one; tm only grows by additions of a positive
 *    finite td; tn = t0 + tm_a is finite plus (finite or one infinity).  d has a component of
 *    magnitude >= 0.57 whose axis clips, and the a0 axis (or, for t0 = 0, every axis) has a p
 *    inside the grid up to rounding, so the smallest tm is finite and the stepped axis moves.
 *    The walk ends within 3 n_l steps: every step moves one axis by s_a = +-1, never back, and an
 *    axis leaves [0, n_l) at its n_l-th step at the latest, so at most 3 (n_l - 1) + 1 cells are
 *    tested.  The cap bounds the loop in the kernel and in the reference alike and is never
 *    reached by legal arithmetic.
 *  Solid.  Occupancy (level 0 only): K1's occupancy bit of the cell.  Alpha: T.a > 0 for the
 *    level-l texel T of the cell, of any of the six faces on an anisotropic level >= 1 (a NaN
 *    alpha is not > 0).
 *  Colour of the hit cell c (the view):
 *    RADIANCE  C = T.rgb at level 0 or in an isotropic pyramid; on an anisotropic level >= 1, with
 *              f_c from d_c >= 0.0f and wd_c = d_c * d_c (A.5's faces and weights of direction d),
 *              per channel  C = fmaf(wd_z, T_fz, fmaf(wd_y, T_fy, wd_x * T_fx)),  exactly as "cone
 *              queries" combines a corner texel
 *    ALPHA     the alpha of the same combination in all three channels
 *    ALBEDO    albedo_occ.rgb of the voxel
 *    NORMAL    fmaf(0.5f, n_c, 0.5f) of the voxel's normal
 *    shade == 1:  C_c = C_c * k with k = VCT_VOXVIEW_SHADE_X, _Y or _Z for face >> 1 = 0, 1, 2 and
 *    1.0f for face 6;  shade == 0 multiplies nothing.
 *    linear4 = (C, 1.0f) on a hit, (+0, +0, +0, +0) on a miss.  rgba8 on a hit, alpha 255:
 *    RADIANCE q(tone(C_c)), the composites' present step ("volumetric fog", Apply); the other
 *    modes q(C_c) without the tone curve (they are not radiance).  rgba8 = 0 on a miss.
 *  Skipping loads.  A form that tests fewer cells' texels must keep every step's arithmetic
 *    (K2's discipline with its coarse bits).  In alpha mode K4's empty-space maps (b0, occ and the
 *    zmaps of vct_internal.h) may be used while they describe the pyramid: they are built from the bit pattern of whole texels
 *    (a texel that is not +0 in all four channels sets its bit), so a clear bit proves every face
 *    of every texel below it +0, hence alpha = +0, not > 0, not solid.  The library's kernels
 *    take the plain walk.
 *  The section's literals (VCT_VOXVIEW_SHADE_X / _Y / _Z, VCT_VOXVIEW_STEPS_PER_CELL) stand with
 *    the present step's, above. */

/* ---- environment sky (vct_set_env / vct_env_*_device / vct_inject_env, include/vct_env.h;
 *      tests/env_ref.py restates it) ------------------------------------------------------------
 *  All arithmetic is float32, one rounding per operation, no contraction; the fused operations
 *    are the fmaf() calls named here.  dot3 is "local lights"'.
 *  The map: S x S RGBA texels, S = 2^lgS, 1 <= S <= VCT_ENV_MAX_DIM (2048), octahedral, row 0 =
 *    p.y = -1; texel (x, y) of level j is M_j[y][x].  Input rule of a texel: r, g, b finite, sign
 *    bit clear (-0.0f is refused), <= VCT_ENV_TEXEL_LIMIT = 2^52; alpha is carried through the
 *    mip rule and never read.  Level j has S_j = S >> j texels per side, j = 0 .. lgS, and per
 *    channel
 *      M_{j+1}[y][x] = ((M_j[2y][2x] + M_j[2y][2x+1]) + (M_j[2y+1][2x] + M_j[2y+1][2x+1])) * 0.25f
 *    (three adds, one multiply).  A constant map is that constant at every level (2c, 4c and
 *    c are exact below 2^54).
 *  The record (frame, scale): every component of frame finite; with the dot products taken in
 *    double, |frame[i].frame[i] - 1| <= VCT_GBUF_ORTHO_EPS and |frame[i].frame[j]| <=
 *    VCT_GBUF_ORTHO_EPS (the camera's rule of the "G-buffer input rule"; handedness is not
 *    tested); scale finite, sign bit clear, <= VCT_ENV_TEXEL_LIMIT.
 *  Env(d, tau), for any direction d and any tau:
 *    1. e_c = dot3(frame[c], d), c = x, y, z;  s = (|e.x| + |e.y|) + |e.z|.
 *       Degenerate: unless s > 0 and s < +inf (a NaN, infinite or zero d, or an overflowing
 *       sum), E = M_lgS[0][0], the map's mean, whatever tau is; go to step 5's last line.  This
 *       is the counterpart of "sky light"'s horizon colour for a NaN u.
 *    2. p = (e.x / s, e.y / s).  If e.z < 0.0f (-0.0f is not):
 *         p = ((1.0f - |p.y|) * copysignf(1.0f, p.x), (1.0f - |p.x|) * copysignf(1.0f, p.y))
 *       both components from the unfolded p.  |p_c| <= 1.
 *    3. x = fminf(fmaxf(tau * (float)S, 1.0f), (float)S);  m = fminf(spec_log2(x), (float)lgS)
 *       (A.6's spec_log2);  j0 = (int)m;  fr = m - (float)j0.  A NaN or negative tau gives x = 1,
 *       m = 0; tau >= 1 gives m = lgS (spec_log2 of a power of two is exact).  m is what
 *       vct_env_lookup_device returns in out4.w, for a degenerate d too.
 *    4. B_j, the bilinear sample of level j, per channel:
 *         u = (p.x * 0.5f + 0.5f) * (float)S_j - 0.5f;  v likewise from p.y
 *         i0 = floorf(u), fu = u - i0;  k0 = floorf(v), fv = v - k0     (-1 <= i0, k0 <= S_j - 1)
 *         a = T(i0, k0), b = T(i0 + 1, k0), c = T(i0, k0 + 1), d = T(i0 + 1, k0 + 1)
 *         t0 = fmaf(fu, b - a, a);  t1 = fmaf(fu, d - c, c);  B_j = fmaf(fv, t1 - t0, t0)
 *       T(x, y), a tap at integer (x, y): xc = min(max(x, 0), S_j - 1), yc likewise;
 *         T(x, y) = M_j[x == xc ? yc : S_j - 1 - yc][y == yc ? xc : S_j - 1 - xc]
 *       i.e. a tap whose x lies outside [0, S_j) takes x clamped and y mirrored, a tap whose y
 *       lies outside takes y clamped and x mirrored, and a tap outside in both (a corner) takes
 *       both mirrors.  That is the octahedral fold: the texel across an edge of the square is
 *       the one mirrored along that edge, so no level has a seam.
 *    5. E = B_j0;  if fr > 0 and j0 < lgS:  E = fmaf(fr, B_{j0+1} - B_j0, B_j0)  (per channel).
 *       Env_c = E_c * scale.
 *    A constant map c returns c * scale in every bit at every d and tau: b - a = +0, so every
 *    fmaf returns its addend.
 *  Bound: a fmaf(f, y - x, x) with 0 <= f < 1 lies within one rounding of [x, y], so
 *    E <= 2^52 (1 + 2^-21) and Env <= 2^104 (1 + 2^-21) < VCT_COLOR_LIMIT = 2^105: the bound
 *    argument of "sky light" (A * Sk below 2^15 * 2^105 * ~3 < 2^122; level 0 stays finite)
 *    carries over unchanged.
 *  vct_env_cones_device / vct_inject_env: "sky light" with its receiver, cones, a_k and T_k
 *    unchanged, and
 *      acc_c = fmaf(w_k * T_k, Env_c(d_k, tau_set), acc_c);   vis = fmaf(w_k, T_k, vis)
 *    tau_set = VCT_TAN30 for 1 and 9 cones, VCT_TAN20 for 16 (the set's aperture: one level pair
 *    per context).  A non-finite d_k takes the degenerate branch.  The diffuse add and the
 *    per-voxel L_c = L_c + A_c * Sk_c are "sky light"'s.
 *  vct_env_specular_device: "sky in view"'s specular cone unchanged, S_c = T * Env_c(r, tau)
 *    with the pixel's clamped tau (the aperture and the level pair are per lane).
 *  vct_env_background_device: "sky in view"'s background with c = Env(d, 0.0f) (level 0).
 *  With a constant map c, scale = 1 and any legal frame each of the four equals its vct_sky
 *    counterpart with zenith = horizon = ground = c in every bit (Sky_c = (c + 0 * s_up) + 0 *
 *    s_dn = c for finite s).
 *  The section's literal (VCT_ENV_TEXEL_LIMIT) stands with VCT_COLOR_LIMIT, above. */

/* ---- shading attributes (vct_set_shading / vct_gbuffer_shaded_device /
 * vct_specular_tint_device, include/vct_shading.h; tests/shading_ref.py restates it) ----------
 *  Input rule, vct_set_shading.  VCT_ESTATE without a voxelization.  VCT_EINVAL, the previous
 *    set kept: NULL verts, idx or materials, n_materials == 0; n_idx != 3 x the static
 *    voxelization's triangles (a dynamic layer's are not counted); an idx[i] >= n_verts; a
 *    present offset (!= VCT_SHADING_NO_ATTR) that is not a multiple of 4 or with offset + size
 *    > vertex_stride (size 12 for normal, tangent, bitangent; 8 for uv); tri_material[t] >=
 *    n_materials; a ks component not finite, with its sign bit set, or > VCT_COLOR_LIMIT (the
 *    colour rule of "K2 input rule"); roughness not in [0, 1] (a NaN fails the compare); a map
 *    index < -1 or >= the texture count of the moment; a flag bit other than
 *    VCT_SHADING_FLIP_GREEN; reserved != 0.  Vertex attribute contents are data, never a status.
 *    The set belongs to the static triangles: vct_voxelize* and vct_load_grid drop it,
 *    vct_voxelize_dynamic* keeps it.
 *  Input rule, vct_gbuffer_shaded_device.  The "G-buffer input rule" on the camera and the frame;
 *    pos4, nrm4, alb4, ks4 not NULL and 16-byte aligned; geo4 (16), tri_id (4), bary2 (8 bytes)
 *    aligned when given: VCT_EINVAL, nothing written.  VCT_ESTATE without a set.
 *  The pixel.  Each written operation rounds once; fmaf appears only where written; dot3(a, b) =
 *    (a.x b.x + a.y b.y) + a.z b.z.  The hit (k, t), pos4, the depth test and the background
 *    texel are vct_gbuffer_raster_device's in every bit.  For a hit on triangle k < the set's
 *    triangle count, with the unit ray direction d:
 *    1. (b1, b2) = the Moller-Trumbore (u, v) of the hit (ray_tri_bary: the operations of the
 *       intersection test).  An attribute a with vertex values a0, a1, a2 interpolates as
 *         a = fmaf(b2, a2 - a0, fmaf(b1, a1 - a0, a0))            ("diffuse maps"' TexCoords form)
 *    2. Ng = the face normal as the raster pass computes and flips it: n = e1 x e2, n / sqrtf(
 *       dot3(n, n)) per component, negated when dot3(n, d) > 0; `flipped` = it was negated.
 *    3. unit(v) = v / sqrtf(dot3(v, v)) per component, defined where dot3(v, v) is finite and
 *       > 0.  N0 = unit(interpolated Normal), negated when flipped; N0 = Ng when the normal
 *       attribute is absent or unit() is not defined.
 *    4. If the material's normal_map is >= 0 and < the CURRENT texture count, and the uv, tangent
 *       and bitangent attributes are present: c = T_map(u, v) ("diffuse maps", rgb);
 *       m = fmaf(2.0f, c, -1.0f) per channel, m.y = -m.y under VCT_SHADING_FLIP_GREEN; T, B = the
 *       interpolated Tangent and Bitangent (not re-orthogonalised), negated when flipped;
 *         N1 = unit((m.x T + m.y B) + m.z N0)  per component,   N1 = N0 where unit() is not defined.
 *       Otherwise N1 = N0.
 *    5. N = N1 if dot3(N1, d) < 0, else Ng: a shading normal never faces away from the viewer.
 *    6. nrm4 = (N, 0); geo4 = (Ng, 0); alb4 = (Kd x T_diffuse as the raster pass, the material's
 *       roughness); ks4 = (Ks_c * T_specular(u, v)_c, 1) where the material's specular_map is
 *       >= 0 and < the current texture count and uv is present, else (Ks, 1); tri_id = k;
 *       bary2 = (b1, b2).
 *    7. A hit outside the set (a dynamic-layer triangle) is the flat record: nrm4 = geo4 = (Ng, 0),
 *       alb4.w = the call's roughness, ks4 = (1, 1, 1, 1); tri_id and bary2 as in 6.
 *    8. Background: pos4 = nrm4 = geo4 = ks4 = 0, alb4 = (0, 0, 0, roughness), tri_id =
 *       0xFFFFFFFF, bary2 = 0.
 *    With every attribute absent and every material's roughness the call's, pos4, nrm4 and alb4
 *    equal vct_gbuffer_raster_device's in every bit.
 *  vct_specular_tint_device: out.rgb = spec.rgb * ks.rgb, out.a = spec.a; contents are data.
 *  No new literal. */

/* ---- present (vct_luminance_meter_device / vct_exposure_update_device / vct_bloom_device /
 * vct_present_device, include/vct_present.h; tests/present_ref.py restates it) ----------------
 *  Each written operation rounds once; fmaf appears only where written.  A pixel p = (r, g, b, a)
 *  of the linear frame is a BACKGROUND pixel when a == 0 (also -0.0f).
 *    Y(p) = fmaf(0.0722f, b, fmaf(0.7152f, g, 0.2126f * r))
 *  Meter.  A background pixel is counted nowhere.  A Y that is NaN, +-Inf or has its sign bit set
 *    (also -0.0f) is `rejected`.  Otherwise key = bits(Y) >> 19,
 *      bin = clamp(key - VCT_PRESENT_KEY0, 0, VCT_PRESENT_BINS - 1),  hist[bin] += 1, counted += 1,
 *    under += 1 where key < VCT_PRESENT_KEY0, over += 1 where key - VCT_PRESENT_KEY0 >
 *    VCT_PRESENT_BINS - 1.  Integer sums: exact, whatever the order.
 *  Exposure update, 64-bit unsigned integers (the division truncates):
 *    counted = counts[0];  lo = counted * low_permille / 1000;  hi = counted * high_permille / 1000
 *    for b = 0 .. 511:       t = min(hist[b], lo);  keep[b] = hist[b] - t;  lo -= t
 *    for b = 511 .. 0:       t = min(keep[b], hi);  keep[b] -= t;           hi -= t
 *    n = sum keep[b];   S = sum b * keep[b];   M = (S * 256) / n          (n > 0)
 *    mean = float_from_bits((VCT_PRESENT_KEY0 << 19) + (M << 11) + (1 << 18))
 *    target = key_value / mean;  target = target < min_exposure ? min_exposure : (target >
 *      max_exposure ? max_exposure : target)
 *    prev = the previous record's exposure where a record is given and that value is finite and
 *      > 0; otherwise there is no prev.
 *    n == 0:                 exposure = target = prev, or 1.0f without one; mean = +0
 *    no prev:                exposure = target
 *    else: rate = target > prev ? rate_up : rate_down;
 *          exposure = rate == 1.0f ? target : prev + (target - prev) * rate
 *    out_state = {exposure, target, mean, (uint32_t)counted}
 *  Bloom.  Level 0 is the frame (w_0 x h_0); level k is w_k = (w_{k-1} + 1) / 2 by h_k likewise;
 *    the last level L is the first of params.levels and the level that is 1 x 1.  A tap (x, y) of
 *    a level outside it is the tap at (min(x, w_k - 1), min(y, h_k - 1)) (and max(., 0)).
 *    The contribution c(p) of a frame pixel, with E the exposure:
 *      Ye = Y(p) * E;  wgt = Ye > 0 ? fmaxf(Ye - threshold, 0) / Ye : 0;  c = (r * wgt, g * wgt, b * wgt)
 *      c = (+0, +0, +0) for a background pixel and where wgt or any channel of c is not finite.
 *    box(t00, t10, t01, t11) = ((t00 + t10) + (t01 + t11)) * 0.25f per channel, t_ij the tap at
 *      (2x + i, 2y + j) of the finer level.
 *    D_1 = box of c over the frame;  D_k = box of D_{k-1}  (k = 2 .. L);  .w of every level is +0.
 *    up2(P)(x, y), P of size pw x ph:  nx = x >> 1, fx = nx + ((x & 1) ? 1 : -1), ny and fy
 *      likewise; with lerp(a, b) = fmaf(b - a, 0.25f, a):
 *        up2 = lerp(lerp(P(nx, ny), P(fx, ny)), lerp(P(nx, fy), P(fx, fy)))
 *      -- the 2x bilinear with weights 9, 3, 3, 1 over 16; a constant plane gives the constant.
 *    U_L = D_L;  U_k = D_k + up2(U_{k+1})  (k = L - 1 .. 1).
 *  Present.  E = the record's exposure when a record is given, else params.exposure.  Per channel
 *    c of a pixel that is not a background pixel:
 *      v = c * E;  with bloom: v = fmaf(up2(U_1)(x, y)_c, bloom_intensity, v)
 *      v = v > 0 ? v : +0            (NaN, negatives and -0.0f)
 *      d = 1.0f where v == +Inf, otherwise by the curve:
 *        REINHARD         d = v / (1.0f + v)
 *        REINHARD_WHITE   d = (v * (1.0f + v / (W * W))) / (1.0f + v);  d = d < 1.0f ? d : 1.0f
 *        ACES             d = (v * fmaf(2.51f, v, 0.03f)) / fmaf(v, fmaf(2.43f, v, 0.59f), 0.14f);
 *                         d = d < 1.0f ? d : 1.0f
 *        CLAMP            d = v < 1.0f ? v : 1.0f
 *      out_display4 = (d_r, d_g, d_b, a)
 *      t = powf(d, VCT_INV_GAMMA)                                         (GAMMA22)
 *      t = d <= 0.0031308f ? d * 12.92f : fmaf(1.055f, powf(d, VCT_SRGB_INV_GAMMA), -0.055f)   (SRGB)
 *      byte = clamp(lroundf(t * 255.0f), 0, 255)                           (dither == 0: quant8)
 *      byte = clamp((int)floorf(fmaf(t, 255.0f, (B[y & 3][x & 3] + 0.5f) / 16.0f)), 0, 255)
 *        with B = {{0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}}       (dither == 1)
 *      out_rgba8 = r | g << 8 | b << 16 | 255 << 24
 *    A background pixel: out_display4 = (VCT_CLEAR_R, VCT_CLEAR_G, VCT_CLEAR_B, a) and out_rgba8 =
 *    lroundf(VCT_CLEAR_c * 255.0f) per channel, alpha 255: the composites' clear colour, outside
 *    exposure, bloom, curve, transfer and dither.
 *    With E = 1 from params, no bloom, REINHARD, GAMMA22 and no dither the bytes are the
 *    composites' own (tone01 and quant8 of csrc/vct_view.h) for every finite radiance >= 0.
 *  The section's literals (VCT_PRESENT_KEY0, VCT_SRGB_INV_GAMMA, VCT_EXPOSURE_LIMIT) stand with
 *  VCT_INV_GAMMA, above. */

/* ---- cutouts (vct_voxelize_cutout* / vct_gbuffer_cutout_device, include/vct_cutout.h;
 * tests/cutout_ref.py restates it) ---------------------------------------------------------------
 *  A binary alpha test: a point of a masked triangle exists or it does not.
 *  M_c(u, v), c = 0 .. 3 (r, g, b, a): the formula T(u, v) of "diffuse maps", unchanged, on
 *    channel c of the RGBA8 texel: the same wrap, texel-centre convention and lerp(a, b, f) =
 *    fmaf(f, b - a, a); texel value byte / 255.0f; a non-finite coordinate becomes 0; base level
 *    only.
 *  A material is MASKED when its vct_cutout entry has map >= 0.  A point of one of its triangles
 *    with TexCoords (u, v) is COVERED iff M_channel(u, v) >= cutoff, compared in float32 (the
 *    texels are bytes, so M is never a NaN).  A masked triangle whose vertex record holds no
 *    TexCoords (uv_offset not a multiple of 4, or uv_offset + 8 > vertex_stride) is opaque.
 *  Input rule, the table (host memory, checked before any launch).  VCT_EINVAL, the context --
 *    the previous grid and mesh included -- left as it was: map < -1 or >= the texture count;
 *    channel > 3; a cutoff that is not finite or outside 0 < cutoff <= 1; reserved != 0; a table
 *    with n_materials == 0.  Every other input: the rules of vct_voxelize_textured*, but that with
 *    a table that masks a material tri_material[t] >= n_materials is K1's index error whether
 *    or not a Kd table or a diffuse-map table is given (the table is indexed by the material).
 *  K1.  A (triangle, voxel) pair of a masked triangle that passes the 13-axis SAT contributes iff
 *    the point K1 uses for the diffuse map -- (b1, b2) of the voxel centre projected onto the plane
 *    and clamped into the triangle, uv = the TexCoords form, both of "diffuse maps" -- is
 *    covered.  A pair that is not covered adds nothing: no sums, no count, no occupancy bit.  A
 *    covered pair adds what vct_voxelize_textured adds (Kd x diffuse map, or Kd).  Candidate
 *    counts and offsets are taken before the SAT and do not change.  Only integer pair sums
 *    enter, so the grid is exact whatever the order.
 *  G-buffer.  A candidate (triangle k, t) of a pixel's ray is ACCEPTED iff t > 0 and triangle k is
 *    opaque or the point at the Moller-Trumbore (b1, b2) of that hit (ray_tri_bary) is covered.
 *    The pixel's hit is the smallest accepted t, ties to the lower triangle index.  near / far
 *    are then tested on that one hit, as the "G-buffer input rule" says: an accepted hit nearer
 *    than near still hides what is behind it, a rejected candidate hides nothing.  The records
 *    are those of vct_gbuffer_raster_device (flat) or "shading attributes" (shaded) for that
 *    (k, t).  A mask index >= the CURRENT texture count (a later, smaller vct_set_textures) is no
 *    mask: the shading rule for a stale map.  Dynamic-layer triangles are opaque.
 *  No new literal. */

/* ---- object motion (vct_objects_poses_device / vct_objects_motion_device, include/vct_motion.h;
 * tests/motion_ref.py restates it) ------------------------------------------------------------------
 *  The set remembers, per object, the last pose an update gave it, all 20 words as given (the
 *    device form's visible and reserved words included); all zero before the first one, so a
 *    never-posed object has visible == 0.  vct_objects_poses_device copies these n_objects records.
 *  Input rule, vct_objects_motion_device (host memory, checked before any launch; nothing is
 *    written).  VCT_EINVAL: NULL pos4, tri_id, bary2, prev_poses or motion4; pos4, nrm4, motion4,
 *    prev_nrm4 or prev_poses not 16-byte aligned, bary2 not 8-byte, tri_id or stats not 4-byte;
 *    width or height 0, above 65536, or more than 2^31 - 1 pixels (the temporal call's limits);
 *    exactly one of nrm4 and prev_nrm4 given; n_prev != the set's n_objects (tested after the
 *    state).  VCT_ESTATE: no set is defined.  Pixel contents, ids, barycentrics and matrix contents
 *    are data, never a status.
 *  The pixel.  float32, one rounding per operation, fmaf only where written; dot3 and unit() are
 *    those of "shading attributes", the transform rule that of "dynamic objects".  n_static = the
 *    static triangles, n_set = the set's, first[o] = object o's first triangle within the set,
 *    k = tri_id, (b1, b2) = bary2, cur[o] = the set's pose of object o, prev = prev_poses.
 *    1. pos4.w == 0: motion4 = prev_nrm4 = +0; the pixel is in no count.
 *    2. k >= n_static + n_set (0xFFFFFFFF included): motion4 = 0, prev_nrm4 = nrm4; APPEARED.
 *    3. k < n_static: the static record, motion4 = (pos4.xyz, 1.0f), prev_nrm4 = nrm4, bit for bit;
 *       STILL.
 *    4. Otherwise o = the last object with first[o] <= k - n_static (an object without triangles
 *       is never the last one), and
 *       a. prev[o].visible == 0: motion4 = 0, prev_nrm4 = nrm4; APPEARED.
 *       b. m[j] of cur[o] and prev[o] have the same bits for the twelve j the transform rule reads
 *          (j % 4 != 3; so -0.0f differs from +0.0f, and a NaN equals itself): the static record;
 *          STILL.  cur[o].visible is not read: no pass writes the id of a hidden object's triangle.
 *       c. Else, with v_i the triangle's object-space vertices (i = 0, 1, 2, in index order),
 *          p_i = the transform rule on v_i with prev[o].m, c_i = the same with cur[o].m:
 *            q = fmaf(b2, p_2 - p_0, fmaf(b1, p_1 - p_0, p_0))    per component ("diffuse maps" form)
 *          motion4 = (q, 1.0f), MOVED, where the three components of q are finite; else
 *          motion4 = 0, APPEARED.
 *          face(a) = e1 x e2 with e1 = a_1 - a_0, e2 = a_2 - a_0 and the cross product of
 *          "shading attributes" step 2 (x = e1.y e2.z - e1.z e2.y, ...): n' = unit(face(p)),
 *          n = unit(face(c)).  Where both are defined, prev_nrm4 = (n', 0), negated when
 *          dot3(n, nrm4.xyz) < 0 (the pass had flipped the face normal towards the viewer; a NaN
 *          compares false); where either is not, prev_nrm4 = nrm4.  prev_nrm4 does not depend on
 *          whether q is finite.
 *  stats = {valid, STILL, MOVED, APPEARED} over the frame, valid = the sum of the other three;
 *    written, not accumulated.
 *  Consequences.  With no object moved since the snapshot every valid pixel has the static record,
 *    and vct_temporal_accumulate_device gives with that motion4 what it gives with motion4 == NULL,
 *    in every bit.  For a rigid motion q is the point the pixel's surface point was at, and n' the
 *    normal it had: with prev_nrm4 as the accumulate's nrm4 its normal test compares last frame's
 *    normal with last frame's G-buffer and its plane test measures along that normal, whatever
 *    the rotation.
 *  No new literal. */
#endif /* VCT_SPEC_H */
