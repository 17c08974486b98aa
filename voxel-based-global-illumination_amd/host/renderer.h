// renderer.h — the reference's renderer plug-in slot and the VCT implementation.
//
// `Renderer` is assets/code/renderer/renderer.h:3-10 unchanged in shape: one
// argument-less virtual called once per frame (engine.cpp:151).
// `ConeTraceRenderer` is the drop-in that replaces the forward GL draw of
// VoxelizationRenderer::Render (r_voxelization.cpp:4-35) with the C-ABI of
// include/vct.h: on the first frame (or when the scene/light changes) it runs
// K1 voxelize -> K2 inject -> K3 mips (-> `bounces` light bounces), and every frame it builds the G-buffer
// from the active camera and runs K4.  An optional dynamic model moves without that: when its
// matrix changed, vct_voxelize_dynamic replaces the layer, then inject -> mips as above.  State is pulled from the registry the
// way the reference pulls programs/models/camera from its singletons.
#pragma once
#include <string>
#include <vector>

#include "vct.h"

namespace vcthost {

class Renderer {
public:
    virtual ~Renderer() = default;
    virtual void Render() = 0;
};

struct ConeTraceSettings {
    uint32_t grid = 256;
    uint32_t width = 800, height = 600;   // reference window size, engine.cpp:52
    uint32_t n_diffuse = 9;
    bool specular = true;
    bool aniso = true;
    float light_dir[3] = {0.3f, 1.0f, 0.2f};
    float light_color[3] = {1.0f, 1.0f, 1.0f};
    float roughness = 0.1f;
    float aabb_min[3] = {-1.0f, -1.0f, -1.0f};
    float extent = 2.0f;
    uint32_t devices = 1;                 // > 1: one context over that many GPUs (vct_create_multi)
    uint32_t bounces = 0;                 // light bounces added to the grid after each inject + build
                                          // (vct_inject_bounces; 0: direct light only)
    // a light list (include/vct_lights.h): when non-empty it replaces light_dir / light_color
    // in K2 (vct_inject_lights) and in the composite (vct_composite_lights_device)
    std::vector<vct_light> lights;
    // > 0: the composite's direct term is shadowed by cones of this half-angle tangent toward
    // every light of the frame (include/vct_shadow.h) instead of the hard voxel walk; 0: the walk
    float shadow_tan = 0.0f;
    // 2 or 4: the frame is traced by vct_trace_mixed_device (include/vct_mixed.h) at that factor
    // with the header's default parameters -- diffuse cones on the low frame and the holes,
    // the specular cone at full resolution; 0: vct_trace_device
    uint32_t mixed_factor = 0;
    // > 0: volumetric fog (include/vct_fog.h) of this density per world unit, the other fields
    // of the medium at the header's defaults: the scatter volume is built from the frame's
    // lights after every relight, and every composite is followed by the view-ray march and
    // the apply; 0: no fog, the frame is the surface composite's
    float fog_density = 0.0f;
    // > 0: temporal accumulation (include/vct_temporal.h) of the diffuse plane over a running
    // mean of at most this many frames (max_len, 1 .. VCT_TEMPORAL_MAX_LEN), the other
    // parameters at the header's defaults: after K4 (and the sky) every frame blends its
    // diffuse plane with the reprojected history of the previous Render(), and the composite
    // reads the accumulated plane; 0: every frame stands alone
    uint32_t temporal_len = 0;
    // > 0: a probes^3 grid of ambient-cube probes (include/vct_query.h; 1 .. VCT_PROBE_MAX_DIM) over
    // the grid's AABB, the first and last probe half a spacing inside it: built at the end of every
    // relight, sampled at the frame's G-buffer by every composite, which then reads that plane in
    // place of K4's diffuse plane (and of the accumulated one); 0: K4's diffuse plane
    uint32_t probes = 0;
    // a sky (include/vct_sky.h): injected per voxel after the mips and before the bounces
    // (vct_inject_sky), and added per pixel to the diffuse plane after K4 (vct_sky_cones_device),
    // so every composite shows it through albedo x diffuse
    bool has_sky = false;
    vct_sky sky = {{0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    // the sky in view (include/vct_sky_view.h; needs has_sky): the sky is also added to the specular
    // plane after K4 (vct_sky_specular_device), and every composite is followed by
    // vct_sky_background_device, so the background shows the sky instead of the clear colour
    bool sky_view = false;
    // the shading G-buffer (include/vct_shading.h): vertex normals, normal and specular maps, Ks and
    // a roughness per material from the loader, and the specular plane tinted by Ks x map_Ks
    bool shaded = false;
    // alpha cutouts (include/vct_cutout.h): > 0 = the cutoff.  A material with a map_d is cut by it
    // (channel 3 of a four-channel file, else channel 0), one without by the alpha of a four-channel
    // map_Kd (vct_host.h has the rule); the model goes through vct_voxelize_cutout and the frame
    // through vct_gbuffer_cutout_device when a material is masked.  0: the mask is ignored
    float cutout = 0.0f;
    // an environment map (include/vct_env.h): env_size^2 RGBA float texels, octahedral, uploaded
    // once with vct_set_env.  It takes the sky's place in every call above: vct_inject_env,
    // vct_env_cones_device and, with sky_view, vct_env_specular_device and
    // vct_env_background_device.  The default frame puts the map's +z at the world's +y
    bool has_env = false;
    std::vector<float> env_texels;
    uint32_t env_size = 0;
    vct_env_sky env = {{{1.0f, 0.0f, 0.0f}, {0.0f, 0.0f, -1.0f}, {0.0f, 1.0f, 0.0f}}, 1.0f};
    // the HDR present (include/vct_present.h): WritePPM takes the composite's linear frame through
    // vct_present_device -- with present_auto the exposure is metered from the frame
    // (vct_luminance_meter_device, vct_exposure_update_device: key 0.18, 100 / 20 permille trimmed,
    // 2^-12 .. 2^12), with present_bloom five levels of vct_bloom_device (threshold 1, intensity
    // 0.25) are added; gamma 2.2, no dither, W = 4 -- instead of the composite's own RGBA8
    bool present = false;
    uint32_t present_curve = 0;           // VCT_CURVE_*
    bool present_auto = false;
    float present_exposure = 1.0f;
    bool present_bloom = false;
    // model matrix applied to the model's vertices before K1, column-major; main.cpp
    // sets the reference's T(0,-1.75,0) S(0.2) (r_voxelization.cpp:26-29) by default
    float model[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    // a dynamic object (include/vct_dynamic.h): the registry name of a second model (empty:
    // none) that is voxelized as the context's dynamic layer with its own model matrix.  When
    // only that matrix changes (SetDynamicMatrix) the frame pays vct_voxelize_dynamic, the
    // inject and the mips, not K1 over the static scene.  Its materials are Kd only
    std::string dynamic_model;
    float dynamic_matrix[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    // rigid objects (include/vct_objects.h): registry names of further models, each with its
    // own model matrix.  They are registered once after a voxelization, in object space; a
    // frame then pays vct_objects_update for the objects whose matrix changed
    // (SetObjectMatrix), the inject and the mips.  The device applies the matrix.  Kd materials
    // only; exclusive with dynamic_model
    struct Object {
        std::string model;
        float matrix[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    };
    std::vector<Object> objects;
    // with temporal_len > 0, shaded and objects: run vct_objects_motion_device every frame and hand
    // its planes to the accumulate (include/vct_motion.h).  false: the accumulate runs without
    // them, as if nothing had moved -- for comparing the two
    bool object_motion = true;
};

class ConeTraceRenderer : public Renderer {
public:
    ConeTraceRenderer(const std::string& model_name, const ConeTraceSettings& s);
    ~ConeTraceRenderer() override;
    void Render() override;

    void MarkSceneDirty() { scene_dirty_ = true; }
    // move the dynamic object: the next Render() replaces the layer and relights
    void SetDynamicMatrix(const float m[16]);
    // move object i of ConeTraceSettings::objects: the next Render() updates it alone and relights
    void SetObjectMatrix(size_t i, const float m[16]);
    bool ok() const { return status_ == VCT_OK; }
    const std::string& error() const { return error_; }
    double last_trace_ms() const { return last_ms_; }
    unsigned long long last_cone_steps() const { return last_steps_; }
    // object motion ran in the last Render() (below); its {valid, static_or_unmoved, moved, appeared}
    bool last_motion(uint32_t out[4]) const { for (int k = 0; k < 4; ++k) out[k] = motion_stats_[k]; return motion_ran_; }
    // composite + present (vct_composite_device: direct + albedo * indirect + specular) -> binary PPM
    // With ConeTraceSettings::present the bytes are vct_present_device's, and a path ending in .png
    // is written as a PNG (RGB)
    bool WritePPM(const std::string& path);
    // the same composite before tone mapping: width x height x 4 float32, row 0 = top, raw little-endian
    bool WriteLinear(const std::string& path);
    // the voxel view (include/vct_voxview.h) of the last Render()'s camera at `level` in `mode`
    // (VCT_VOXVIEW_*), shaded by entry face, at the frame's size -> PNG (RGB)
    bool WriteVoxelView(const std::string& path, uint32_t level, uint32_t mode);

private:
    bool check(vct_status s, const char* what);
    bool rebuild_scene();
    bool update_dynamic();                // the dynamic model, placed by its matrix, as the context's layer
    bool define_objects();                // the settings' objects as the context's set, all placed
    bool update_objects();                // vct_objects_update of the objects whose matrix changed
    bool relight();                       // inject -> mips (-> sky, bounces), as after every voxelization
    // row f3 into `lin` (float4) or `rgba` (packed 8-bit), with the light list when there is one
    vct_status composite(float* lin, uint32_t* rgba);
    vct_status present_frame(const float* lin, uint32_t* rgba);  // the settings' present of a linear frame
    vct_status composite_surface(float* lin, uint32_t* rgba);   // the composite without the fog (with the sky behind it: sky_view)
    vct_status composite_terms(float* lin, uint32_t* rgba);     // direct + albedo * diffuse + specular by the frame's lights
    std::vector<vct_light> frame_lights() const;                // the light list, or the default light as one
    vct_fog fog() const;                                        // fog_density with the header defaults
    vct_probe_grid probe_grid() const;                          // the probes^3 grid over the AABB

    std::string model_name_;
    ConeTraceSettings s_;
    vct_ctx* ctx_ = nullptr;
    void* gb_[3] = {nullptr, nullptr, nullptr};
    void* out_[2] = {nullptr, nullptr};
    void* counter_ = nullptr;
    void* vis_ = nullptr;                 // V planes of the soft-shadow composite (shadow_tan > 0), kept
    size_t vis_bytes_ = 0;
    void* sky_ = nullptr;                 // (Sk.rgb, vis) plane of the frame's sky call (has_sky), kept
    void* ks_ = nullptr;                  // (Ks x map_Ks, 1) plane of the shaded G-buffer pass (shaded), kept
    void* sky_spec_ = nullptr;            // (S.rgb, T) plane of the frame's specular sky call (sky_view), kept
    void* probes_ = nullptr;              // probes, states and the sampled plane of the probe grid (probes > 0), kept
    void* probe_state_ = nullptr;
    void* probe_plane_ = nullptr;
    void* fog_ = nullptr;                 // ray, fog and linear planes of the fog pass (fog_density > 0), kept
    vct_camera cam_{};                    // the camera of the last Render(), for the fog's background rays
    // temporal accumulation (temporal_len > 0): the accumulated diffuse planes and history lengths of
    // this frame and the last one (hist_cur_: this frame's), and the last frame's position and normal
    // planes and camera; gb_[0..1] and prev_gb_ swap every frame instead of being copied
    bool accumulate_diffuse();
    void* hist_[2] = {nullptr, nullptr};
    void* hist_len_[2] = {nullptr, nullptr};
    void* prev_gb_[2] = {nullptr, nullptr};
    vct_camera prev_cam_{};
    bool has_prev_ = false;               // prev_gb_, prev_cam_ and hist_[1 - hist_cur_] hold a frame
    int hist_cur_ = 0;
    // object motion (include/vct_motion.h), with temporal_len > 0, shaded and a set of objects: the
    // shaded pass also writes tri_id and bary2, vct_objects_motion_device turns them and the pose
    // snapshot of the last frame's end into motion4 and the previous-pose normal plane, the
    // accumulate reads both, and the snapshot is taken again after it
    bool object_motion();
    void* tri_id_ = nullptr;
    void* bary_ = nullptr;
    void* motion_ = nullptr;
    void* pnrm_ = nullptr;
    void* pose_snap_ = nullptr;
    void* motion_stats_dev_ = nullptr;
    size_t snap_objects_ = 0;             // records pose_snap_ holds
    bool has_snap_ = false;               // pose_snap_ holds the poses of the last frame's end, of this set
    bool motion_ran_ = false;             // motion_ and pnrm_ are this frame's
    uint32_t motion_stats_[4] = {0, 0, 0, 0};
    bool scene_dirty_ = true;
    bool dynamic_dirty_ = true;           // the dynamic matrix changed since the layer was voxelized
    std::vector<char> object_dirty_;      // per object: its matrix changed since the last update
    vct_status status_ = VCT_OK;
    std::string error_;
    double last_ms_ = 0.0;
    unsigned long long last_steps_ = 0;
};

}  // namespace vcthost
