// main.cpp — headless equivalent of the reference's main()/Engine::RenderLoop
// (core/main.cpp:4-27, engine.cpp:140-157).  No GLFW/GL context exists in this
// image, so the loop runs a fixed number of frames and
// dumps the last one as a PPM instead of swapping buffers.
//
//   vct_headless <model.obj> [grid=256] [width=800] [height=600] [frames=5] [out.ppm] [devices=1]
//                [--model=reference|identity] [--grid=fit|unit] [--bounces N] [--linear=frame.f32]
//                [--light SPEC]... [--shadow-tan T] [--sky Z[:H[:G]]] [--env FILE[:SCALE]] [--sky-view] [--mixed 2|4]
//                [--fog DENSITY] [--temporal N] [--probes D] [--present CURVE[:auto|:E][:bloom]]
//                [--dynamic FILE.obj [--dynamic-offset x,y,z]]
//                [--object FILE.obj[@x,y,z]]... [--object-step x,y,z] [--no-object-motion]
//                [--voxels LEVEL[:MODE]]...
//   (devices > 1: one process drives that many GPUs through vct_create_multi)
//   --model: the model matrix of the reference's draw, T(0,-1.75,0) S(0.2)
//            (r_voxelization.cpp:26-29; default), or none;
//   --grid:  the cubic grid around the placed model's bounds with one voxel of
//            padding (default), or [-1,1]^3 padded by one voxel (unit-box scenes).
//   --bounces: light bounces added to the grid after each inject + build
//            (vct_inject_bounces; default 0);
//   --linear: also dump the last frame before tone mapping (raw float32 [h][w][4]).
//   --shadow-tan: T > 0 shades the direct term with shadow cones of half-angle tangent T toward
//            every light of the frame (include/vct_shadow.h) instead of the hard voxel walk;
//            0 (the default) keeps the walk;
//   --sky:    a sky (include/vct_sky.h) with up = +y: Z, H and G are the r,g,b of the zenith, the
//            horizon (default: Z) and the ground (default: 0,0,0).  It is injected per voxel
//            after the mips and before the bounces, and added per pixel to the diffuse term;
//   --sky-view: with --sky, the sky in view (include/vct_sky_view.h): the sky is also seen by the
//            specular cone of every pixel, and the background shows it instead of the clear colour;
//   --env:    FILE[:SCALE]: an environment map (include/vct_env.h) in the sky's place: FILE is raw
//            little-endian float32 RGBA texels of an octahedral square, S from the file size (S * S
//            * 16 bytes, S a power of two <= 2048; any other size is a usage error), the map's +z at
//            the world's +y, SCALE (default 1) its intensity.  It replaces --sky in the per-voxel
//            inject and the diffuse call and, with --sky-view, in the specular and background calls;
//   --mixed:  2 or 4: the frame is traced at mixed resolution (include/vct_mixed.h): diffuse cones on
//            a frame that many times smaller per axis, upsampled, holes traced exactly, the
//            specular cone at full resolution; absent: the full-resolution trace;
//   --fog:    DENSITY > 0: volumetric fog (include/vct_fog.h) of that extinction per world unit, the
//            other fields of the medium at the header's defaults: the scatter volume is built
//            from the frame's lights, and the frame is the composite seen through the march;
//   --temporal: N in 1 .. 1024: temporal accumulation (include/vct_temporal.h): every frame blends its
//            diffuse plane with the reprojected history of the frame before it, a running mean of at
//            most N frames, the other parameters at the header's defaults, and the composite reads
//            the accumulated plane; absent: every frame stands alone;
//   --probes: D in 1 .. 256: a D^3 grid of ambient-cube probes (include/vct_query.h) over the grid's
//            AABB, built after every relight; the composite reads the probe-sampled plane in place of
//            K4's diffuse plane (the specular cone is still traced); absent: K4's diffuse plane;
//   --present: CURVE[:auto|:E][:bloom], CURVE one of reinhard, white, aces, clamp: the frame is written
//            through the HDR present (include/vct_present.h) of the composite's linear frame in place of
//            the composite's own RGBA8 -- at the manual exposure E (default 1), or metered from the
//            frame (auto), with five levels of bloom on request -- and as a PNG when the output path
//            ends in .png; gamma 2.2, no dither.  `reinhard` alone gives the composite's bytes;
//   --voxels: LEVEL[:MODE], repeatable: after the last frame, the voxel view (include/vct_voxview.h) of
//            the frame's camera through pyramid level LEVEL is written next to the frame as
//            <out stem>.voxels<LEVEL>-<MODE>.png, shaded by entry face.  MODE: radiance (default),
//            alpha, albedo or normal; albedo and normal exist at level 0 only;
//   --shaded: the shading G-buffer (include/vct_shading.h): the loader's vertex normals, tangents and
//            bitangents, each material's Ks, Ns (as roughness sqrt(2 / (Ns + 2))), map_Ks and normal
//            map (map_Kn, else the map_Bump / bump slot) go through vct_set_shading and
//            vct_gbuffer_shaded_device, and vct_specular_tint_device tints the specular plane before
//            the composite; absent: face normals, one roughness, an untinted specular plane;
//   --cutouts: [=CUTOFF, default 0.5] alpha cutouts (include/vct_cutout.h): a material's map_d (channel 3
//            of a four-channel file, else channel 0), or else the alpha of a four-channel map_Kd, is a
//            binary mask: the model goes through vct_voxelize_cutout and the frame through
//            vct_gbuffer_cutout_device when some material is masked; absent: the masks are ignored;
//   --dynamic: a second model, voxelized as the context's dynamic layer (include/vct_dynamic.h)
//            on top of the first one's grid; Kd materials only (its diffuse maps are not loaded).
//            --dynamic-offset: a world-space translation applied after the model matrix of
//            --model (default 0,0,0).  The grid is fitted to the first model alone;
//   --object: a further model as one rigid object of the context's object set
//            (include/vct_objects.h), repeatable, in set order; @x,y,z: a world-space translation
//            applied after the model matrix of --model.  The set is registered once in object
//            space and the device applies each matrix; Kd materials only.  Exclusive with
//            --dynamic;
//   --object-step: x,y,z: every --object advances by this much per frame (frame f shows it at its
//            offset + f x step; only the moved objects are voxelized again).  With --temporal N and
//            --shaded the frame loop also runs vct_objects_motion_device (include/vct_motion.h) and
//            hands its two planes to the accumulate, so a moving object keeps its history;
//            --no-object-motion leaves that call out (the accumulate then runs as if nothing had
//            moved), for comparing the two;
//   --light:  one light of a light list (include/vct_lights.h), repeatable, in list order; with
//            any --light the list replaces the default directional light.  SPEC is colon-
//            separated fields of comma-separated floats, world units, angles in degrees:
//              dir:dx,dy,dz:r,g,b                     (direction toward the light)
//              point:x,y,z:r,g,b:range
//              spot:x,y,z:dx,dy,dz:r,g,b:range:inner_deg:outer_deg   (d = the axis it shines along)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "assets.h"

using namespace vcthost;

// one --light SPEC (see above) -> *out; false: malformed
static bool parse_light(const std::string& spec, vct_light* out) {
    std::vector<std::vector<float>> f;      // the numeric fields after the type
    std::string type;
    size_t at = 0;
    for (int k = 0; at <= spec.size(); ++k) {
        const size_t end = std::min(spec.find(':', at), spec.size());
        const std::string field = spec.substr(at, end - at);
        at = end + 1;
        if (k == 0) { type = field; continue; }
        std::vector<float> v;
        const char* p = field.c_str();
        while (*p) {
            char* q = nullptr;
            v.push_back(std::strtof(p, &q));
            if (q == p) return false;
            p = *q == ',' ? q + 1 : q;
            if (*q && *q != ',') return false;
        }
        f.push_back(v);
    }
    auto is = [&](size_t i, size_t n) { return i < f.size() && f[i].size() == n; };
    auto put3 = [](float* dst, const std::vector<float>& v) { for (int k = 0; k < 3; ++k) dst[k] = v[k]; };
    *out = vct_light{};
    if (type == "dir" && f.size() == 2 && is(0, 3) && is(1, 3)) {
        out->type = VCT_LIGHT_DIRECTIONAL;
        put3(out->direction, f[0]);
        put3(out->color, f[1]);
    } else if (type == "point" && f.size() == 3 && is(0, 3) && is(1, 3) && is(2, 1)) {
        out->type = VCT_LIGHT_POINT;
        put3(out->position, f[0]);
        put3(out->color, f[1]);
        out->range = f[2][0];
    } else if (type == "spot" && f.size() == 6 && is(0, 3) && is(1, 3) && is(2, 3) && is(3, 1) && is(4, 1) && is(5, 1)) {
        out->type = VCT_LIGHT_SPOT;
        put3(out->position, f[0]);
        put3(out->direction, f[1]);
        put3(out->color, f[2]);
        out->range = f[3][0];
        const float rad = 3.14159265358979323846f / 180.0f;
        out->cos_inner = std::cos(f[4][0] * rad);
        out->cos_outer = std::cos(f[5][0] * rad);
    } else {
        return false;
    }
    return true;
}

// one --sky Z[:H[:G]] (see above) -> *out with up = +y; false: malformed (a field that is not
// three numbers, more than three fields, a negative or non-finite component)
static bool parse_sky(const std::string& spec, vct_sky* out) {
    float c[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    size_t at = 0;
    int k = 0;
    for (; at <= spec.size(); ++k) {
        if (k == 3) return false;
        const size_t end = std::min(spec.find(':', at), spec.size());
        const std::string field = spec.substr(at, end - at);
        at = end + 1;
        const char* p = field.c_str();
        for (int j = 0; j < 3; ++j) {
            char* q = nullptr;
            c[k][j] = std::strtof(p, &q);
            if (q == p || *q != (j < 2 ? ',' : '\0')) return false;
            if (!std::isfinite(c[k][j]) || std::signbit(c[k][j])) return false;
            p = q + 1;
        }
    }
    *out = vct_sky{};
    out->up[1] = 1.0f;
    for (int j = 0; j < 3; ++j) {
        out->zenith[j] = c[0][j];
        out->horizon[j] = k > 1 ? c[1][j] : c[0][j];
        out->ground[j] = k > 2 ? c[2][j] : 0.0f;
    }
    return true;
}

// one --env FILE[:SCALE] (see above) -> the texels, their size and the scale; false, with *why:
// a file that cannot be read or whose size is not S * S * 16 bytes for a power of two S in
// 1 .. VCT_ENV_MAX_DIM, or a SCALE that is not a finite number >= 0.  A suffix after the last ':'
// that is not a number belongs to the file name.
static bool parse_env(const std::string& spec, std::vector<float>* texels, uint32_t* size, float* scale,
                      std::string* why) {
    std::string file = spec;
    *scale = 1.0f;
    const size_t colon = spec.rfind(':');
    if (colon != std::string::npos && colon + 1 < spec.size()) {
        const std::string tail = spec.substr(colon + 1);
        char* end = nullptr;
        const float v = std::strtof(tail.c_str(), &end);
        if (end != tail.c_str() && *end == '\0') {
            if (!std::isfinite(v) || std::signbit(v)) { *why = "SCALE must be finite and >= 0"; return false; }
            *scale = v;
            file = spec.substr(0, colon);
        }
    }
    std::FILE* f = std::fopen(file.c_str(), "rb");
    if (!f) { *why = "cannot open " + file; return false; }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    uint32_t s = 0;
    for (uint32_t k = 1; k <= VCT_ENV_MAX_DIM; k <<= 1)
        if (bytes == (long)k * (long)k * 16) s = k;
    if (!s) {
        std::fclose(f);
        *why = file + ": " + std::to_string(bytes) + " bytes is not S*S*16 for a power of two S <= " + std::to_string(VCT_ENV_MAX_DIM);
        return false;
    }
    texels->resize((size_t)s * s * 4);
    const size_t got = std::fread(texels->data(), 16, (size_t)s * s, f);
    std::fclose(f);
    if (got != (size_t)s * s) { *why = "short read of " + file; return false; }
    *size = s;
    return true;
}

// one --voxels LEVEL[:MODE] (see above); false: malformed
struct VoxelView {
    uint32_t level, mode;
    std::string mode_name;
};
static bool parse_voxels(const std::string& spec, VoxelView* out) {
    static const char* const names[4] = {"radiance", "alpha", "albedo", "normal"};   // VCT_VOXVIEW_* order
    const size_t colon = spec.find(':');
    const std::string lv = spec.substr(0, colon);
    out->mode_name = colon == std::string::npos ? "radiance" : spec.substr(colon + 1);
    char* end = nullptr;
    const long l = std::strtol(lv.c_str(), &end, 10);
    if (lv.empty() || lv[0] < '0' || lv[0] > '9' || *end || l > 10) return false;
    out->level = (uint32_t)l;
    for (uint32_t m = 0; m < 4; ++m)
        if (out->mode_name == names[m]) {
            out->mode = m;
            return m < VCT_VOXVIEW_ALBEDO || l == 0;
        }
    return false;
}

// --present CURVE[:auto|:E][:bloom] (see above); false: malformed
struct PresentSpec {
    bool on = false, automatic = false, bloom = false;
    uint32_t curve = VCT_CURVE_REINHARD;
    float exposure = 1.0f;
};
static bool parse_present(const std::string& spec, PresentSpec* out) {
    static const char* const names[4] = {"reinhard", "white", "aces", "clamp"};   // VCT_CURVE_* order
    std::vector<std::string> tok;
    for (size_t at = 0;;) {
        const size_t colon = spec.find(':', at);
        tok.push_back(spec.substr(at, colon == std::string::npos ? colon : colon - at));
        if (colon == std::string::npos) break;
        at = colon + 1;
    }
    PresentSpec p;
    uint32_t c = 0;
    while (c < 4 && tok[0] != names[c]) ++c;
    if (c == 4 || tok.size() > 3) return false;
    p.curve = c;
    size_t i = 1;
    if (i < tok.size() && tok[i] != "bloom") {
        if (tok[i] == "auto") p.automatic = true;
        else {
            char* end = nullptr;
            p.exposure = std::strtof(tok[i].c_str(), &end);
            const char f = tok[i].empty() ? '\0' : tok[i][0];
            if (!((f >= '0' && f <= '9') || f == '.') || *end || !(p.exposure > 0.0f) || !(p.exposure <= 18446744073709551616.0f))
                return false;
        }
        ++i;
    }
    if (i < tok.size()) {
        if (tok[i] != "bloom") return false;
        p.bloom = true;
        ++i;
    }
    if (i != tok.size()) return false;
    p.on = true;
    *out = p;
    return true;
}

// one --dynamic-offset x,y,z -> out[3]; false: malformed (not exactly three finite numbers)
static bool parse_offset(const std::string& spec, float out[3]) {
    const char* p = spec.c_str();
    for (int j = 0; j < 3; ++j) {
        char* q = nullptr;
        out[j] = std::strtof(p, &q);
        if (q == p || *q != (j < 2 ? ',' : '\0') || !std::isfinite(out[j])) return false;
        p = q + 1;
    }
    return true;
}

int main(int argc, char** argv) {
    std::vector<std::string> pos;
    std::string dynamic;
    bool has_dynamic = false, has_offset = false;
    float dyn_offset[3] = {0.0f, 0.0f, 0.0f};
    struct ObjectArg { std::string file; float offset[3]; };
    std::vector<ObjectArg> objects;
    float object_step[3] = {0.0f, 0.0f, 0.0f};
    bool has_step = false, object_motion = true;
    bool ref_model = true, fit_grid = true;
    int bounces = 0;
    std::string linear;
    std::vector<vct_light> lights;
    float shadow_tan = 0.0f;
    bool has_sky = false, sky_view = false, shaded = false;
    float cutout = 0.0f;
    vct_sky sky{};
    bool has_env = false;
    std::vector<float> env_texels;
    uint32_t env_size = 0;
    float env_scale = 1.0f;
    uint32_t mixed = 0;
    float fog_density = 0.0f;
    uint32_t temporal = 0;
    uint32_t probes = 0;
    PresentSpec present;
    std::vector<VoxelView> voxels;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--model=reference") ref_model = true;
        else if (a == "--model=identity") ref_model = false;
        else if (a == "--grid=fit") fit_grid = true;
        else if (a == "--grid=unit") fit_grid = false;
        else if (a == "--bounces" && i + 1 < argc) bounces = std::atoi(argv[++i]);
        else if (a.rfind("--bounces=", 0) == 0) bounces = std::atoi(a.c_str() + 10);
        else if (a.rfind("--linear=", 0) == 0) linear = a.substr(9);
        else if (a == "--shadow-tan" && i + 1 < argc) shadow_tan = std::strtof(argv[++i], nullptr);
        else if (a.rfind("--shadow-tan=", 0) == 0) shadow_tan = std::strtof(a.c_str() + 13, nullptr);
        else if ((a == "--light" && i + 1 < argc) || a.rfind("--light=", 0) == 0) {
            const std::string spec = a == "--light" ? argv[++i] : a.substr(8);
            vct_light l;
            if (!parse_light(spec, &l)) { std::fprintf(stderr, "malformed --light %s\n", spec.c_str()); return 2; }
            lights.push_back(l);
        }
        else if ((a == "--sky" && i + 1 < argc) || a.rfind("--sky=", 0) == 0) {
            const std::string spec = a == "--sky" ? argv[++i] : a.substr(6);
            if (!parse_sky(spec, &sky)) { std::fprintf(stderr, "malformed --sky %s\n", spec.c_str()); return 2; }
            has_sky = true;
        }
        else if (a == "--sky-view") sky_view = true;
        else if (a == "--shaded") shaded = true;
        else if (a == "--cutouts") cutout = 0.5f;
        else if (a.rfind("--cutouts=", 0) == 0) cutout = (float)atof(a.c_str() + 10);
        else if (a == "--env" || a.rfind("--env=", 0) == 0) {
            const std::string spec = a == "--env" ? (i + 1 < argc ? argv[++i] : "") : a.substr(6);
            std::string why;
            if (spec.empty() || !parse_env(spec, &env_texels, &env_size, &env_scale, &why)) {
                std::fprintf(stderr, "malformed --env %s (%s)\n", spec.c_str(), spec.empty() ? "FILE[:SCALE]" : why.c_str());
                return 2;
            }
            has_env = true;
        }
        else if (a == "--mixed" || a.rfind("--mixed=", 0) == 0) {
            const std::string v = a == "--mixed" ? (i + 1 < argc ? argv[++i] : "") : a.substr(8);
            if (v != "2" && v != "4") { std::fprintf(stderr, "malformed --mixed %s (2 or 4)\n", v.c_str()); return 2; }
            mixed = (uint32_t)(v[0] - '0');
        }
        else if (a == "--fog" || a.rfind("--fog=", 0) == 0) {
            const std::string v = a == "--fog" ? (i + 1 < argc ? argv[++i] : "") : a.substr(6);
            char* end = nullptr;
            fog_density = std::strtof(v.c_str(), &end);
            if (v.empty() || *end || !(fog_density > 0.0f) || !std::isfinite(fog_density)) {
                std::fprintf(stderr, "malformed --fog %s (a density > 0)\n", v.c_str());
                return 2;
            }
        }
        else if (a == "--temporal" || a.rfind("--temporal=", 0) == 0) {
            const std::string v = a == "--temporal" ? (i + 1 < argc ? argv[++i] : "") : a.substr(11);
            char* end = nullptr;
            const long t = std::strtol(v.c_str(), &end, 10);
            if (v.empty() || v[0] < '0' || v[0] > '9' || *end || t < 1 || t > (long)VCT_TEMPORAL_MAX_LEN) {
                std::fprintf(stderr, "malformed --temporal %s (1 .. %u)\n", v.c_str(), VCT_TEMPORAL_MAX_LEN);
                return 2;
            }
            temporal = (uint32_t)t;
        }
        else if (a == "--present" || a.rfind("--present=", 0) == 0) {
            const std::string v = a == "--present" ? (i + 1 < argc ? argv[++i] : "") : a.substr(10);
            if (!parse_present(v, &present)) {
                std::fprintf(stderr, "malformed --present %s (reinhard|white|aces|clamp[:auto|:E][:bloom], 0 < E <= 2^64)\n", v.c_str());
                return 2;
            }
        }
        else if (a == "--probes" || a.rfind("--probes=", 0) == 0) {
            const std::string v = a == "--probes" ? (i + 1 < argc ? argv[++i] : "") : a.substr(9);
            char* end = nullptr;
            const long d = std::strtol(v.c_str(), &end, 10);
            if (v.empty() || v[0] < '0' || v[0] > '9' || *end || d < 1 || d > (long)VCT_PROBE_MAX_DIM) {
                std::fprintf(stderr, "malformed --probes %s (1 .. %d)\n", v.c_str(), VCT_PROBE_MAX_DIM);
                return 2;
            }
            probes = (uint32_t)d;
        }
        else if (a == "--voxels" || a.rfind("--voxels=", 0) == 0) {
            const std::string v = a == "--voxels" ? (i + 1 < argc ? argv[++i] : "") : a.substr(9);
            VoxelView vv;
            if (!parse_voxels(v, &vv)) {
                std::fprintf(stderr, "malformed --voxels %s (LEVEL[:radiance|alpha|albedo|normal]; albedo and normal at level 0)\n", v.c_str());
                return 2;
            }
            voxels.push_back(vv);
        }
        else if (a == "--dynamic-offset" || a.rfind("--dynamic-offset=", 0) == 0) {
            const std::string spec = a == "--dynamic-offset" ? (i + 1 < argc ? argv[++i] : "") : a.substr(17);
            if (!parse_offset(spec, dyn_offset)) { std::fprintf(stderr, "malformed --dynamic-offset %s\n", spec.c_str()); return 2; }
            has_offset = true;
        }
        else if (a == "--dynamic" || a.rfind("--dynamic=", 0) == 0) {
            dynamic = a == "--dynamic" ? (i + 1 < argc ? argv[++i] : "") : a.substr(10);
            if (dynamic.empty() || dynamic.rfind("--", 0) == 0) { std::fprintf(stderr, "--dynamic needs a file (--dynamic FILE.obj)\n"); return 2; }
            has_dynamic = true;
        }
        else if (a == "--no-object-motion") object_motion = false;
        else if (a == "--object-step" || a.rfind("--object-step=", 0) == 0) {
            const std::string spec = a == "--object-step" ? (i + 1 < argc ? argv[++i] : "") : a.substr(14);
            if (!parse_offset(spec, object_step)) { std::fprintf(stderr, "malformed --object-step %s\n", spec.c_str()); return 2; }
            has_step = true;
        }
        else if (a == "--object" || a.rfind("--object=", 0) == 0) {
            const std::string spec = a == "--object" ? (i + 1 < argc ? argv[++i] : "") : a.substr(9);
            ObjectArg o{spec.substr(0, spec.rfind('@')), {0.0f, 0.0f, 0.0f}};
            if (o.file.empty() || o.file.rfind("--", 0) == 0) { std::fprintf(stderr, "--object needs a file (--object FILE.obj[@x,y,z])\n"); return 2; }
            if (spec.rfind('@') != std::string::npos && !parse_offset(spec.substr(spec.rfind('@') + 1), o.offset)) {
                std::fprintf(stderr, "malformed --object offset %s\n", spec.c_str());
                return 2;
            }
            objects.push_back(o);
        }
        else if (a.rfind("--", 0) == 0) { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
        else pos.push_back(a);
    }
    if (sky_view && !has_sky && !has_env) { std::fprintf(stderr, "--sky-view needs --sky Z[:H[:G]] or --env FILE[:SCALE]\n"); return 2; }
    if (pos.empty()) {
        std::fprintf(stderr, "usage: %s model.obj [grid] [width] [height] [frames] [out.ppm] [devices] "
                             "[--model=reference|identity] [--grid=fit|unit] [--bounces N] [--linear=frame.f32] [--shadow-tan T] [--sky Z[:H[:G]]] [--env FILE[:SCALE]] [--sky-view] [--shaded] [--cutouts[=CUTOFF]] [--mixed 2|4] [--fog DENSITY] [--temporal N] [--probes D] [--present CURVE[:auto|:E][:bloom]] [--voxels LEVEL[:MODE]]... "
                             "[--dynamic FILE.obj [--dynamic-offset x,y,z]] [--object FILE.obj[@x,y,z]]... [--object-step x,y,z] [--no-object-motion] "
                             "[--light dir:d:rgb | point:p:rgb:range | spot:p:d:rgb:range:inner:outer]...\n",
                     argv[0]);
        return 2;
    }
    ConeTraceSettings s;
    if (pos.size() > 1) s.grid = (uint32_t)std::atoi(pos[1].c_str());
    if (pos.size() > 2) s.width = (uint32_t)std::atoi(pos[2].c_str());
    if (pos.size() > 3) s.height = (uint32_t)std::atoi(pos[3].c_str());
    const int frames = pos.size() > 4 ? std::atoi(pos[4].c_str()) : 5;
    const std::string out = pos.size() > 5 ? pos[5] : "vct_frame.ppm";
    if (pos.size() > 6) s.devices = (uint32_t)std::atoi(pos[6].c_str());
    if (s.grid < 4) { std::fprintf(stderr, "grid must be >= 4\n"); return 2; }
    if (bounces < 0) { std::fprintf(stderr, "--bounces must be >= 0\n"); return 2; }
    if (!(shadow_tan >= 0.0f) || !std::isfinite(shadow_tan)) { std::fprintf(stderr, "--shadow-tan must be finite and >= 0\n"); return 2; }
    if (has_offset && !has_dynamic) { std::fprintf(stderr, "--dynamic-offset needs --dynamic FILE.obj\n"); return 2; }
    if (has_dynamic && !objects.empty()) { std::fprintf(stderr, "--object and --dynamic exclude each other\n"); return 2; }
    if (has_step && objects.empty()) { std::fprintf(stderr, "--object-step needs --object FILE.obj[@x,y,z]\n"); return 2; }
    s.bounces = (uint32_t)bounces;
    s.shadow_tan = shadow_tan;
    s.lights = lights;
    s.has_sky = has_sky;
    s.sky = sky;
    s.sky_view = sky_view;
    s.shaded = shaded;
    s.cutout = cutout;
    s.has_env = has_env;
    s.env_texels = std::move(env_texels);
    s.env_size = env_size;
    s.env.scale = env_scale;
    s.mixed_factor = mixed;
    s.fog_density = fog_density;
    s.temporal_len = temporal;
    s.object_motion = object_motion;
    s.probes = probes;
    s.present = present.on;
    s.present_curve = present.curve;
    s.present_auto = present.automatic;
    s.present_exposure = present.exposure;
    s.present_bloom = present.bloom;
    if (ref_model) ReferenceModelMatrix(s.model);

    AssetsManager& A = AssetsManager::Instance();            // assets.cpp:22-45
    A.cameras["FPS"] = std::make_shared<Camera>(0.0f, 0.0f, 3.0f);
    auto model = std::make_shared<Model>();
    std::string err;
    if (!model->LoadObj(pos[0], &err)) {
        std::fprintf(stderr, "ERROR::OBJ:: %s\n", err.c_str());   // model.cpp:25-29
        return 1;
    }
    for (const std::string& e : model->texture_errors)            // model.cpp:219-223
        std::printf("Texture failed to load at path: %s\n", e.c_str());
    std::printf("%zu diffuse maps\n", model->textures.size());
    float lo[3], hi[3];
    Model placed = *model;
    placed.Transform(s.model);
    if (fit_grid && placed.Bounds(lo, hi)) {
        GridForBounds(lo, hi, s.grid, s.aabb_min, &s.extent);
    } else {   // [-1,1]^3 padded by one voxel (vct.scenes.grid_for_unit_box)
        s.extent = 2.0f * s.grid / (s.grid - 2);
        for (float& a : s.aabb_min) a = -s.extent / 2;
    }
    std::printf("grid %u: aabb_min %a %a %a extent %a\n", s.grid, (double)s.aabb_min[0], (double)s.aabb_min[1],
                (double)s.aabb_min[2], (double)s.extent);
    A.models["test"] = model;
    if (has_dynamic) {   // the dynamic object: the same model matrix, then the world-space offset
        auto dyn = std::make_shared<Model>();
        if (!dyn->LoadObj(dynamic, &err, false)) {
            std::fprintf(stderr, "ERROR::OBJ:: %s\n", err.c_str());
            return 1;
        }
        A.models["dynamic"] = dyn;
        s.dynamic_model = "dynamic";
        for (int i = 0; i < 16; ++i) s.dynamic_matrix[i] = s.model[i];
        for (int k = 0; k < 3; ++k) s.dynamic_matrix[12 + k] = s.model[12 + k] + dyn_offset[k];
    }
    for (size_t k = 0; k < objects.size(); ++k) {   // rigid objects: the same model matrix, then each one's offset
        auto obj = std::make_shared<Model>();
        if (!obj->LoadObj(objects[k].file, &err, false)) {
            std::fprintf(stderr, "ERROR::OBJ:: %s\n", err.c_str());
            return 1;
        }
        ConeTraceSettings::Object o;
        o.model = "object" + std::to_string(k);
        A.models[o.model] = obj;
        for (int i = 0; i < 16; ++i) o.matrix[i] = s.model[i];
        for (int j = 0; j < 3; ++j) o.matrix[12 + j] = s.model[12 + j] + objects[k].offset[j];
        s.objects.push_back(o);
    }
    auto r = std::make_shared<ConeTraceRenderer>("test", s);
    A.renderers["ConeTrace"] = r;
    for (int f = 0; f < frames; ++f) {
        if (has_step && f > 0) {   // every object advances by the step: frame f shows offset + f * step
            for (size_t k = 0; k < s.objects.size(); ++k) {
                float m[16];
                for (int i = 0; i < 16; ++i) m[i] = s.objects[k].matrix[i];
                for (int j = 0; j < 3; ++j) m[12 + j] = s.objects[k].matrix[12 + j] + (float)f * object_step[j];
                r->SetObjectMatrix(k, m);
            }
        }
        A.renderers["ConeTrace"]->Render();                   // engine.cpp:151
        if (!r->ok()) return 1;
        std::printf("frame %d: K4 %.3f ms, %llu cone steps, %.1f Mcone-steps/s\n", f, r->last_trace_ms(),
                    r->last_cone_steps(), r->last_cone_steps() / (r->last_trace_ms() * 1e3));
        uint32_t ms[4];
        if (r->last_motion(ms))    // object motion ran (--temporal, --shaded and --object together)
            std::printf("frame %d: motion valid %u still %u moved %u appeared %u\n", f, ms[0], ms[1], ms[2], ms[3]);
    }
    if (!r->WritePPM(out)) return 1;
    if (!linear.empty() && !r->WriteLinear(linear)) return 1;
    std::printf("wrote %s\n", out.c_str());
    for (const VoxelView& v : voxels) {
        const size_t dot = out.rfind('.'), slash = out.rfind('/');
        const std::string stem = dot != std::string::npos && (slash == std::string::npos || dot > slash) ? out.substr(0, dot) : out;
        const std::string png = stem + ".voxels" + std::to_string(v.level) + "-" + v.mode_name + ".png";
        if (!r->WriteVoxelView(png, v.level, v.mode)) {
            std::fprintf(stderr, "voxel view %u:%s failed: %s\n", v.level, v.mode_name.c_str(), r->error().c_str());
            return 1;
        }
        std::printf("wrote %s\n", png.c_str());
    }
    return 0;
}
