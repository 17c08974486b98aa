// renderer.cpp — ConeTraceRenderer: the reference's Renderer slot driving the VCT C-ABI.
#include "renderer.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "assets.h"
#include "png.h"

namespace vcthost {

ConeTraceRenderer::ConeTraceRenderer(const std::string& model_name, const ConeTraceSettings& s)
    : model_name_(model_name), s_(s) {
    vct_config cfg{};
    cfg.n = s.grid;
    for (int k = 0; k < 3; ++k) cfg.aabb_min[k] = s.aabb_min[k];
    cfg.extent = s.extent;
    cfg.aniso = s.aniso ? 1 : 0;
    cfg.n_diffuse = s.n_diffuse;
    cfg.specular = s.specular ? 1 : 0;
    cfg.device = -1;
    if (!check(s.devices > 1 ? vct_create_multi(&cfg, s.devices, &ctx_) : vct_create(&cfg, &ctx_), "vct_create"))
        return;
    const size_t fb = (size_t)s.width * s.height * 16;
    for (auto& p : gb_)
        if (!check(vct_device_alloc(ctx_, fb, &p), "alloc gbuffer")) return;
    for (auto& p : out_)
        if (!check(vct_device_alloc(ctx_, fb, &p), "alloc output")) return;
    if (!check(vct_device_alloc(ctx_, 8, &counter_), "alloc counter")) return;
    if (s.has_env && !check(vct_set_env(ctx_, s.env_texels.data(), s.env_size), "vct_set_env")) return;
    if (s.temporal_len) {
        for (auto& p : hist_)
            if (!check(vct_device_alloc(ctx_, fb, &p), "alloc history plane")) return;
        for (auto& p : hist_len_)
            if (!check(vct_device_alloc(ctx_, fb / 4, &p), "alloc history lengths")) return;
        for (auto& p : prev_gb_)
            if (!check(vct_device_alloc(ctx_, fb, &p), "alloc previous gbuffer")) return;
    }
}

ConeTraceRenderer::~ConeTraceRenderer() {
    if (!ctx_) return;
    for (void* p : gb_) vct_device_free(ctx_, p);
    for (void* p : out_) vct_device_free(ctx_, p);
    vct_device_free(ctx_, counter_);
    if (vis_) vct_device_free(ctx_, vis_);
    if (sky_) vct_device_free(ctx_, sky_);
    if (sky_spec_) vct_device_free(ctx_, sky_spec_);
    if (ks_) vct_device_free(ctx_, ks_);
    if (fog_) vct_device_free(ctx_, fog_);
    for (void* p : {probes_, probe_state_, probe_plane_}) if (p) vct_device_free(ctx_, p);
    for (void* p : hist_) if (p) vct_device_free(ctx_, p);
    for (void* p : hist_len_) if (p) vct_device_free(ctx_, p);
    for (void* p : prev_gb_) if (p) vct_device_free(ctx_, p);
    for (void* p : {tri_id_, bary_, motion_, pnrm_, pose_snap_, motion_stats_dev_}) if (p) vct_device_free(ctx_, p);
    vct_destroy(ctx_);
}

bool ConeTraceRenderer::check(vct_status st, const char* what) {
    if (st == VCT_OK) return true;
    status_ = st;
    error_ = std::string(what) + ": " + vct_status_string(st) + " " + (ctx_ ? vct_last_error(ctx_) : "");
    std::fprintf(stderr, "ConeTraceRenderer: %s\n", error_.c_str());   // reference style: print, continue
    return false;
}

bool ConeTraceRenderer::rebuild_scene() {
    auto model = AssetsManager::Instance().models[model_name_];
    if (!model) { error_ = "no model '" + model_name_ + "'"; return false; }
    std::vector<Vertex> v;
    std::vector<unsigned> idx, tri_mat;
    std::vector<float> kd4;
    Model placed = *model;              // the draw's model matrix, as the GL pass applies it (test.vert)
    placed.Transform(s_.model);
    placed.Flatten(v, idx, tri_mat, kd4);
    // the diffuse maps (Model::loadMaterialTextures): albedo = Kd x map in K1 and the G-buffer
    std::vector<vct_texture> tex;
    for (const Texture& t : model->textures) tex.push_back(vct_texture{t.rgba.data(), t.width, t.height});
    // the shading maps follow the diffuse ones in the one texture set (shaded)
    const int32_t shading_base = (int32_t)tex.size();
    if (s_.shaded || s_.cutout > 0.0f)
        for (const Texture& t : model->shading_textures) tex.push_back(vct_texture{t.rgba.data(), t.width, t.height});
    if (!check(vct_set_textures(ctx_, tex.data(), (uint32_t)tex.size()), "vct_set_textures")) return false;
    const std::vector<int32_t> map = model->MaterialMap();
    // the cutout table (vct_host.h's rule): map_d, else the alpha of a four-channel map_Kd
    std::vector<vct_cutout> cut;
    bool masked = false;
    if (s_.cutout > 0.0f)
        for (const Material& mt : model->materials) {
            vct_cutout c{-1, 0u, s_.cutout, 0u};
            const int od = mt.shadingMaps[kMapOpacity], kd = mt.diffuseMaps.empty() ? -1 : mt.diffuseMaps[0];
            if (od >= 0) {
                c.map = shading_base + od;
                c.channel = model->shading_textures[od].comp == 4 ? 3u : 0u;
            } else if (kd >= 0 && model->textures[kd].comp == 4) {
                c.map = kd;
                c.channel = 3u;
            }
            masked |= c.map >= 0;
            cut.push_back(c);
        }
    if (masked) {
        if (!check(vct_voxelize_cutout(ctx_, v.data(), sizeof(Vertex), (uint32_t)v.size(), idx.data(), (uint32_t)idx.size(),
                                       tri_mat.data(), kd4.data(), map.data(), cut.data(), (uint32_t)(kd4.size() / 4),
                                       (uint32_t)offsetof(Vertex, TexCoords)),
                   "vct_voxelize_cutout"))
            return false;
    } else if (!check(vct_voxelize_textured(ctx_, v.data(), sizeof(Vertex), (uint32_t)v.size(), idx.data(),
                                            (uint32_t)idx.size(), tri_mat.data(), kd4.data(), map.data(),
                                            (uint32_t)(kd4.size() / 4), (uint32_t)offsetof(Vertex, TexCoords)),
                      "vct_voxelize_textured")) {
        return false;
    }
    if (s_.shaded) {
        // Material::Ks, Ns as a roughness, the specular map, and as the normal map the slot the
        // reference reads (map_Kn) or else the height slot (nanosuit's *_ddn.png are normal maps)
        std::vector<vct_shading_material> mats;
        for (const Material& mt : model->materials) {
            vct_shading_material sm{};
            for (int k = 0; k < 3; ++k) sm.ks[k] = mt.Ks[k];
            sm.roughness = std::min(1.0f, std::max(0.0f, std::sqrt(2.0f / (mt.Ns + 2.0f))));
            const int nm = mt.shadingMaps[kMapNormal] >= 0 ? mt.shadingMaps[kMapNormal] : mt.shadingMaps[kMapHeight];
            sm.normal_map = nm >= 0 ? shading_base + nm : -1;
            sm.specular_map = mt.shadingMaps[kMapSpecular] >= 0 ? shading_base + mt.shadingMaps[kMapSpecular] : -1;
            mats.push_back(sm);
        }
        vct_shading_desc d{};
        d.verts = v.data(); d.vertex_stride = sizeof(Vertex); d.n_verts = (uint32_t)v.size();
        d.idx = idx.data(); d.n_idx = (uint32_t)idx.size();
        d.tri_material = tri_mat.data();
        d.normal_offset = (uint32_t)offsetof(Vertex, Normal); d.uv_offset = (uint32_t)offsetof(Vertex, TexCoords);
        d.tangent_offset = (uint32_t)offsetof(Vertex, Tangent); d.bitangent_offset = (uint32_t)offsetof(Vertex, Bitangent);
        d.materials = mats.data(); d.n_materials = (uint32_t)mats.size();
        if (!check(vct_set_shading(ctx_, &d), "vct_set_shading")) return false;
    }
    scene_dirty_ = false;
    dynamic_dirty_ = true;              // a voxelization drops the layer: put it back before the light
    if (!s_.dynamic_model.empty()) return update_dynamic();
    if (!s_.objects.empty()) return define_objects();   // a voxelization drops the set too
    return relight();
}

void ConeTraceRenderer::SetObjectMatrix(size_t i, const float m[16]) {
    if (i >= s_.objects.size() || std::memcmp(s_.objects[i].matrix, m, sizeof s_.objects[i].matrix) == 0) return;
    std::memcpy(s_.objects[i].matrix, m, sizeof s_.objects[i].matrix);
    object_dirty_.resize(s_.objects.size(), 1);
    object_dirty_[i] = 1;
}

bool ConeTraceRenderer::define_objects() {
    // every model in object space, as the loader gives it; one material table for the set: the
    // models' tables back to back
    const size_t n = s_.objects.size();
    std::vector<std::vector<Vertex>> v(n);
    std::vector<std::vector<unsigned>> idx(n), tri_mat(n);
    std::vector<float> kd4;
    std::vector<vct_object_mesh> meshes(n);
    for (size_t k = 0; k < n; ++k) {
        auto model = AssetsManager::Instance().models[s_.objects[k].model];
        if (!model) { error_ = "no model '" + s_.objects[k].model + "'"; status_ = VCT_EINVAL; return false; }
        std::vector<float> kd;
        model->Flatten(v[k], idx[k], tri_mat[k], kd);
        for (unsigned& m : tri_mat[k]) m += (unsigned)(kd4.size() / 4);
        kd4.insert(kd4.end(), kd.begin(), kd.end());
        meshes[k].verts = v[k].data(); meshes[k].vertex_stride = sizeof(Vertex); meshes[k].n_verts = (uint32_t)v[k].size();
        meshes[k].idx = idx[k].data(); meshes[k].n_idx = (uint32_t)idx[k].size();
        meshes[k].tri_material = tri_mat[k].data();
    }
    if (!check(vct_objects_define(ctx_, meshes.data(), (uint32_t)n, kd4.empty() ? nullptr : kd4.data(), (uint32_t)(kd4.size() / 4)),
               "vct_objects_define"))
        return false;
    has_snap_ = false;                  // a new set: the snapshot describes the old one
    object_dirty_.assign(n, 1);
    return update_objects();
}

bool ConeTraceRenderer::update_objects() {
    std::vector<uint32_t> ids;
    std::vector<vct_object_pose> poses;
    for (size_t k = 0; k < s_.objects.size(); ++k) {
        if (!object_dirty_[k]) continue;
        vct_object_pose p{};
        std::memcpy(p.m, s_.objects[k].matrix, sizeof p.m);
        p.visible = 1;
        ids.push_back((uint32_t)k);
        poses.push_back(p);
    }
    if (!check(vct_objects_update(ctx_, ids.data(), poses.data(), (uint32_t)ids.size()), "vct_objects_update")) return false;
    object_dirty_.assign(s_.objects.size(), 0);
    return relight();
}

void ConeTraceRenderer::SetDynamicMatrix(const float m[16]) {
    if (std::memcmp(s_.dynamic_matrix, m, sizeof s_.dynamic_matrix) == 0) return;
    std::memcpy(s_.dynamic_matrix, m, sizeof s_.dynamic_matrix);
    dynamic_dirty_ = true;
}

bool ConeTraceRenderer::update_dynamic() {
    auto model = AssetsManager::Instance().models[s_.dynamic_model];
    if (!model) { error_ = "no model '" + s_.dynamic_model + "'"; status_ = VCT_EINVAL; return false; }
    std::vector<Vertex> v;
    std::vector<unsigned> idx, tri_mat;
    std::vector<float> kd4;
    Model placed = *model;
    placed.Transform(s_.dynamic_matrix);
    placed.Flatten(v, idx, tri_mat, kd4);
    if (!check(vct_voxelize_dynamic(ctx_, v.data(), sizeof(Vertex), (uint32_t)v.size(), idx.data(), (uint32_t)idx.size(),
                                    tri_mat.data(), kd4.data(), (uint32_t)(kd4.size() / 4)),
               "vct_voxelize_dynamic"))
        return false;
    dynamic_dirty_ = false;
    return relight();
}

bool ConeTraceRenderer::relight() {
    if (!s_.lights.empty()) {
        if (!check(vct_inject_lights(ctx_, s_.lights.data(), (uint32_t)s_.lights.size()), "vct_inject_lights"))
            return false;
    } else if (!check(vct_inject_directional(ctx_, s_.light_dir, s_.light_color), "vct_inject_directional")) {
        return false;
    }
    if (!check(vct_build_mips(ctx_), "vct_build_mips")) return false;
    if (s_.has_env) {   // the map takes the sky's place (one of the two per level 0)
        if (!check(vct_inject_env(ctx_, &s_.env), "vct_inject_env")) return false;
    } else if (s_.has_sky && !check(vct_inject_sky(ctx_, &s_.sky), "vct_inject_sky")) {
        return false;
    }
    if (s_.bounces && !check(vct_inject_bounces(ctx_, s_.bounces), "vct_inject_bounces")) return false;
    if (s_.fog_density > 0.0f) {   // the scatter volume of the finished pyramid, one visibility cone per light
        const std::vector<vct_light> lights = frame_lights();
        const std::vector<float> tan_half(lights.size(), VCT_FOG_DEFAULT_TAN);
        const vct_fog f = fog();
        if (!check(vct_build_fog(ctx_, &f, lights.data(), (uint32_t)lights.size(), tan_half.data()), "vct_build_fog"))
            return false;
    }
    if (s_.probes) {   // the probes see the finished pyramid: sky and bounces included
        const size_t n = (size_t)s_.probes * s_.probes * s_.probes;
        if (!probes_ && !check(vct_device_alloc(ctx_, n * 6 * 16, &probes_), "alloc probes")) return false;
        if (!probe_state_ && !check(vct_device_alloc(ctx_, n * 4, &probe_state_), "alloc probe states")) return false;
        const vct_probe_grid pg = probe_grid();
        if (!check(vct_probe_build_device(ctx_, &pg, (float*)probes_, (uint32_t*)probe_state_, nullptr), "vct_probe_build_device"))
            return false;
    }
    return true;
}

vct_probe_grid ConeTraceRenderer::probe_grid() const {
    vct_probe_grid pg{};
    pg.spacing = s_.extent / (float)s_.probes;
    for (int k = 0; k < 3; ++k) {
        pg.origin[k] = s_.aabb_min[k] + 0.5f * pg.spacing;
        pg.dims[k] = s_.probes;
    }
    return pg;
}

std::vector<vct_light> ConeTraceRenderer::frame_lights() const {
    std::vector<vct_light> lights = s_.lights;
    if (lights.empty()) {     // the default directional light as a list of one
        vct_light l{};
        l.type = VCT_LIGHT_DIRECTIONAL;
        for (int k = 0; k < 3; ++k) { l.direction[k] = s_.light_dir[k]; l.color[k] = s_.light_color[k]; }
        lights.push_back(l);
    }
    return lights;
}

vct_fog ConeTraceRenderer::fog() const {
    vct_fog f{};
    f.density = s_.fog_density;
    f.albedo[0] = f.albedo[1] = f.albedo[2] = VCT_FOG_DEFAULT_ALBEDO;
    f.ambient = VCT_FOG_DEFAULT_AMBIENT;
    f.level = s_.grid >= 16u ? VCT_FOG_DEFAULT_LEVEL : 1u;   // a volume needs four cells per axis
    f.step = VCT_FOG_DEFAULT_STEP;
    return f;
}

void ConeTraceRenderer::Render() {
    if (!ctx_ || status_ != VCT_OK) return;
    if (scene_dirty_) {
        if (!rebuild_scene()) return;
    } else if (!s_.dynamic_model.empty() && dynamic_dirty_ && !update_dynamic()) {
        return;
    } else if (std::find(object_dirty_.begin(), object_dirty_.end(), 1) != object_dirty_.end() && !update_objects()) {
        return;
    }
    auto cam = AssetsManager::Instance().ActiveCamera();
    if (!cam) return;
    const vct_camera vc = cam->ToVct();
    cam_ = vc;
    if (s_.temporal_len && has_prev_) {   // the last frame's G-buffer stays; this frame's goes to the other pair
        std::swap(gb_[0], prev_gb_[0]);
        std::swap(gb_[1], prev_gb_[1]);
    }
    if (s_.shaded && !ks_ && !check(vct_device_alloc(ctx_, (size_t)s_.width * s_.height * 16, &ks_), "alloc ks plane")) return;
    const bool track = s_.temporal_len && s_.shaded && !s_.objects.empty() && s_.object_motion;   // object motion (renderer.h)
    if (track && !tri_id_) {
        const size_t px = (size_t)s_.width * s_.height;
        if (!check(vct_device_alloc(ctx_, px * 4, &tri_id_), "alloc tri_id plane") ||
            !check(vct_device_alloc(ctx_, px * 8, &bary_), "alloc bary plane") ||
            !check(vct_device_alloc(ctx_, px * 16, &motion_), "alloc motion plane") ||
            !check(vct_device_alloc(ctx_, px * 16, &pnrm_), "alloc previous-normal plane") ||
            !check(vct_device_alloc(ctx_, 16, &motion_stats_dev_), "alloc motion stats"))
            return;
    }
    uint32_t* const tri_id = track ? (uint32_t*)tri_id_ : nullptr;
    float* const bary = track ? (float*)bary_ : nullptr;
    motion_ran_ = false;
    if (vct_cutout_materials(ctx_) > 0) {   // a cutout mesh: the masked pass, flat or shaded records
        if (!check(vct_gbuffer_cutout_device(ctx_, &vc, s_.width, s_.height, s_.roughness, (float*)gb_[0], (float*)gb_[1],
                                             (float*)gb_[2], s_.shaded ? (float*)ks_ : nullptr, nullptr, tri_id, bary),
                   "cutout G-buffer"))
            return;
    } else if (s_.shaded) {
        if (!check(vct_gbuffer_shaded_device(ctx_, &vc, s_.width, s_.height, s_.roughness, (float*)gb_[0], (float*)gb_[1],
                                             (float*)gb_[2], (float*)ks_, nullptr, tri_id, bary), "shaded G-buffer"))
            return;
    } else if (!check(vct_gbuffer_raster_device(ctx_, &vc, s_.width, s_.height, s_.roughness, (float*)gb_[0],
                                                (float*)gb_[1], (float*)gb_[2]), "G-buffer")) {
        return;
    }
    if (track && has_prev_ && has_snap_ && !object_motion()) return;
    unsigned long long zero = 0;
    if (!check(vct_memcpy(ctx_, counter_, &zero, 8, 0), "reset counter")) return;
    vct_trace_args a{};
    a.pos4 = (const float*)gb_[0];
    a.nrm4 = (const float*)gb_[1];
    a.alb4 = (const float*)gb_[2];
    a.width = s_.width;
    a.height = s_.height;
    for (int k = 0; k < 3; ++k) a.eye[k] = cam->Position[k];
    a.diffuse4 = (float*)out_[0];
    a.spec4 = (float*)out_[1];
    a.cone_steps = (unsigned long long*)counter_;
    auto t0 = std::chrono::steady_clock::now();
    if (s_.mixed_factor) {
        vct_mixed_params mp{};
        if (!check(vct_mixed_default_params(ctx_, s_.mixed_factor, &mp), "vct_mixed_default_params")) return;
        if (!check(vct_trace_mixed_device(ctx_, &a, &mp), "vct_trace_mixed_device")) return;
    } else if (!check(vct_trace_device(ctx_, &a), "vct_trace_device")) {
        return;
    }
    if (!check(vct_synchronize(ctx_), "sync")) return;
    last_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    check(vct_memcpy(ctx_, &last_steps_, counter_, 8, 1), "read counter");
    if (s_.has_sky || s_.has_env) {   // the sky into the diffuse plane, once per frame, before whichever composite reads it
        if (!sky_ && !check(vct_device_alloc(ctx_, (size_t)s_.width * s_.height * 16, &sky_), "alloc sky plane")) return;
        if (s_.has_env)
            check(vct_env_cones_device(ctx_, a.pos4, a.nrm4, s_.width, s_.height, &s_.env, (float*)sky_, a.diffuse4, nullptr),
                  "vct_env_cones_device");
        else
            check(vct_sky_cones_device(ctx_, a.pos4, a.nrm4, s_.width, s_.height, &s_.sky, (float*)sky_, a.diffuse4, nullptr),
                  "vct_sky_cones_device");
    }
    if ((s_.has_sky || s_.has_env) && s_.sky_view && status_ == VCT_OK) {   // and into the specular plane
        if (!sky_spec_ && !check(vct_device_alloc(ctx_, (size_t)s_.width * s_.height * 16, &sky_spec_), "alloc specular sky plane"))
            return;
        if (s_.has_env)
            check(vct_env_specular_device(ctx_, a.pos4, a.nrm4, a.alb4, s_.width, s_.height, a.eye, &s_.env,
                                          (float*)sky_spec_, a.spec4, nullptr),
                  "vct_env_specular_device");
        else
            check(vct_sky_specular_device(ctx_, a.pos4, a.nrm4, a.alb4, s_.width, s_.height, a.eye, &s_.sky,
                                          (float*)sky_spec_, a.spec4, nullptr),
                  "vct_sky_specular_device");
    }
    // the tint goes before any composite, and after everything that adds to the specular plane
    if (s_.shaded && status_ == VCT_OK)
        check(vct_specular_tint_device(ctx_, a.spec4, (const float*)ks_, s_.width, s_.height, a.spec4), "vct_specular_tint_device");
    if (s_.temporal_len && status_ == VCT_OK) accumulate_diffuse();
    if (track && status_ == VCT_OK) {   // the snapshot: this frame's poses are the next frame's previous ones
        if (snap_objects_ < s_.objects.size()) {
            if (pose_snap_) vct_device_free(ctx_, pose_snap_);
            pose_snap_ = nullptr;
            if (!check(vct_device_alloc(ctx_, s_.objects.size() * sizeof(vct_object_pose), &pose_snap_), "alloc pose snapshot")) return;
            snap_objects_ = s_.objects.size();
        }
        if (!check(vct_objects_poses_device(ctx_, (vct_object_pose*)pose_snap_, (uint32_t)snap_objects_), "vct_objects_poses_device"))
            return;
        has_snap_ = true;
        if (motion_ran_) check(vct_memcpy(ctx_, motion_stats_, motion_stats_dev_, 16, 1), "read motion stats");
    }
}

bool ConeTraceRenderer::object_motion() {
    vct_motion_args m{};
    m.width = s_.width;
    m.height = s_.height;
    m.pos4 = (const float*)gb_[0];
    m.nrm4 = (const float*)gb_[1];
    m.tri_id = (const uint32_t*)tri_id_;
    m.bary2 = (const float*)bary_;
    m.prev_poses = (const vct_object_pose*)pose_snap_;
    m.n_prev = (uint32_t)s_.objects.size();
    m.motion4 = (float*)motion_;
    m.prev_nrm4 = (float*)pnrm_;
    m.stats = (uint32_t*)motion_stats_dev_;
    if (!check(vct_objects_motion_device(ctx_, &m), "vct_objects_motion_device")) return false;
    motion_ran_ = true;
    return true;
}

bool ConeTraceRenderer::accumulate_diffuse() {
    vct_temporal_params tp{};
    if (!check(vct_temporal_default_params(ctx_, &tp), "vct_temporal_default_params")) return false;
    tp.max_len = s_.temporal_len;
    const int now = has_prev_ ? 1 - hist_cur_ : hist_cur_;
    vct_temporal_args t{};
    t.width = s_.width;
    t.height = s_.height;
    t.pos4 = (const float*)gb_[0];
    t.nrm4 = (const float*)gb_[1];
    if (motion_ran_) {   // the tap tests read the normals under the last frame's poses; prev_gb_ keeps the real ones
        t.motion4 = (const float*)motion_;
        t.nrm4 = (const float*)pnrm_;
    }
    if (has_prev_) {
        t.prev_cam = &prev_cam_;
        t.prev_pos4 = (const float*)prev_gb_[0];
        t.prev_nrm4 = (const float*)prev_gb_[1];
        t.hist4[0] = (const float*)hist_[1 - now];
        t.hist_len = (const uint32_t*)hist_len_[1 - now];
    }
    t.n_planes = 1;
    t.cur4[0] = (const float*)out_[0];
    t.out4[0] = (float*)hist_[now];
    t.out_len = (uint32_t*)hist_len_[now];
    if (!check(vct_temporal_accumulate_device(ctx_, &t, &tp), "vct_temporal_accumulate_device")) return false;
    prev_cam_ = cam_;
    has_prev_ = true;
    hist_cur_ = now;
    return true;
}

vct_status ConeTraceRenderer::composite(float* lin, uint32_t* rgba) {
    if (!(s_.fog_density > 0.0f)) return composite_surface(lin, rgba);
    // fog: the surface composite's linear frame (ours when the caller only wants RGBA8), then the
    // segments, the march and rgb = rgb * T + F on it
    const size_t plane = (size_t)s_.width * s_.height * 16;
    if (!fog_) {
        const vct_status st = vct_device_alloc(ctx_, 3 * plane, &fog_);
        if (st != VCT_OK) return st;
    }
    float* const ray = (float*)fog_;
    float* const fog4 = (float*)((char*)fog_ + plane);
    float* const frame = lin ? lin : (float*)((char*)fog_ + 2 * plane);
    vct_status st = composite_surface(frame, nullptr);
    if (st != VCT_OK) return st;
    const vct_fog f = fog();
    if ((st = vct_fog_rays_device(ctx_, &cam_, cam_.position, (const float*)gb_[0], s_.width, s_.height, ray)) != VCT_OK)
        return st;
    if ((st = vct_fog_march_device(ctx_, &f, cam_.position, ray, s_.width, s_.height, fog4, nullptr)) != VCT_OK) return st;
    return vct_fog_apply_device(ctx_, fog4, s_.width, s_.height, frame, rgba);
}

vct_status ConeTraceRenderer::composite_surface(float* lin, uint32_t* rgba) {
    const vct_status st = composite_terms(lin, rgba);
    if (st != VCT_OK || !((s_.has_sky || s_.has_env) && s_.sky_view)) return st;
    if (s_.has_env)
        return vct_env_background_device(ctx_, &cam_, (const float*)gb_[0], s_.width, s_.height, &s_.env, lin, rgba);
    return vct_sky_background_device(ctx_, &cam_, (const float*)gb_[0], s_.width, s_.height, &s_.sky, lin, rgba);
}

vct_status ConeTraceRenderer::composite_terms(float* lin, uint32_t* rgba) {
    const float *pos = (const float*)gb_[0], *nrm = (const float*)gb_[1], *alb = (const float*)gb_[2];
    const float* diff = (const float*)(s_.temporal_len && has_prev_ ? hist_[hist_cur_] : out_[0]);   // the accumulated plane
    const float* spec = (const float*)out_[1];
    if (s_.probes) {   // the probe grid lights the frame in place of K4's diffuse cones
        if (!probe_plane_) {
            const vct_status st = vct_device_alloc(ctx_, (size_t)s_.width * s_.height * 16, &probe_plane_);
            if (st != VCT_OK) return st;
        }
        const vct_probe_grid pg = probe_grid();
        const vct_status st = vct_probe_sample_device(ctx_, &pg, (const float*)probes_, (const uint32_t*)probe_state_, pos, nrm,
                                                      s_.width * s_.height, (float*)probe_plane_, nullptr);
        if (st != VCT_OK) return st;
        diff = (const float*)probe_plane_;
    }
    if (s_.shadow_tan > 0.0f) {   // soft shadows: V per (light, pixel) from shadow cones, then the composite over it
        const std::vector<vct_light> lights = frame_lights();
        const std::vector<float> tan_half(lights.size(), s_.shadow_tan);
        const size_t need = lights.size() * (size_t)s_.width * s_.height * sizeof(float);
        if (need > vis_bytes_) {   // the planes stay with the renderer, as gb_ and out_ do
            if (vis_) vct_device_free(ctx_, vis_);
            vis_ = nullptr;
            vis_bytes_ = 0;
            const vct_status st = vct_device_alloc(ctx_, need, &vis_);
            if (st != VCT_OK) return st;
            vis_bytes_ = need;
        }
        const vct_status st = vct_shadow_cones_device(ctx_, pos, nrm, s_.width, s_.height, lights.data(),
                                                      (uint32_t)lights.size(), tan_half.data(), (float*)vis_, nullptr);
        if (st != VCT_OK) return st;
        return vct_composite_shadowed_device(ctx_, pos, nrm, alb, diff, spec, s_.width, s_.height, lights.data(),
                                             (uint32_t)lights.size(), (const float*)vis_, lin, rgba);
    }
    if (!s_.lights.empty())
        return vct_composite_lights_device(ctx_, pos, nrm, alb, diff, spec, s_.width, s_.height, s_.lights.data(),
                                           (uint32_t)s_.lights.size(), lin, rgba);
    return vct_composite_device(ctx_, pos, nrm, alb, diff, spec, s_.width, s_.height, s_.light_dir, s_.light_color,
                                lin, rgba);
}

vct_status ConeTraceRenderer::present_frame(const float* lin, uint32_t* rgba) {
    const uint32_t w = s_.width, h = s_.height;
    // hist[512], counts[4] and the exposure record in one block; the bloom scratch in another
    void *meter = nullptr, *scratch = nullptr;
    vct_status st = vct_device_alloc(ctx_, 512 * 4 + 16 + 16, &meter);
    uint32_t* hist = (uint32_t*)meter;
    uint32_t* counts = hist + 512;
    vct_exposure_state* state = s_.present_auto ? (vct_exposure_state*)(counts + 4) : nullptr;
    if (st == VCT_OK && s_.present_auto) {
        vct_exposure_params e{};
        e.key_value = 0.18f; e.min_exposure = 1.0f / 4096.0f; e.max_exposure = 4096.0f;
        e.low_permille = 100; e.high_permille = 20;
        e.rate_up = e.rate_down = 1.0f;
        st = vct_luminance_meter_device(ctx_, lin, w, h, hist, counts);
        if (st == VCT_OK) st = vct_exposure_update_device(ctx_, hist, counts, &e, nullptr, state);
    }
    if (st == VCT_OK && s_.present_bloom) {
        vct_bloom_params b{};
        b.threshold = 1.0f; b.levels = 5; b.exposure = s_.present_exposure;
        size_t bytes = 0;
        st = vct_bloom_scratch_bytes(w, h, b.levels, &bytes);
        if (st == VCT_OK) st = vct_device_alloc(ctx_, bytes, &scratch);
        if (st == VCT_OK) st = vct_bloom_device(ctx_, lin, w, h, &b, state, (float*)scratch, bytes);
    }
    if (st == VCT_OK) {
        vct_present_params p{};
        p.curve = s_.present_curve; p.transfer = VCT_TRANSFER_GAMMA22; p.dither = 0;
        p.exposure = s_.present_exposure; p.white = 4.0f; p.bloom_intensity = 0.25f;
        st = vct_present_device(ctx_, lin, w, h, &p, state, (const float*)scratch, nullptr, rgba);
    }
    if (st == VCT_OK) st = vct_synchronize(ctx_);      // the blocks below are freed
    if (scratch) vct_device_free(ctx_, scratch);
    if (meter) vct_device_free(ctx_, meter);
    return st;
}

bool ConeTraceRenderer::WritePPM(const std::string& path) {
    // row f3: composite + present on the device (include/vct.h vct_composite_device), then dump
    if (!ctx_) return false;
    const size_t px = (size_t)s_.width * s_.height;
    void *rgba = nullptr, *lin = nullptr;
    if (!check(vct_device_alloc(ctx_, px * 4, &rgba), "alloc rgba8")) return false;
    std::vector<uint32_t> img(px);
    bool ok;
    if (s_.present)
        ok = check(vct_device_alloc(ctx_, px * 16, &lin), "alloc linear frame") && check(composite((float*)lin, nullptr), "composite") &&
             check(present_frame((const float*)lin, (uint32_t*)rgba), "present");
    else
        ok = check(composite(nullptr, (uint32_t*)rgba), "composite");
    ok = ok && check(vct_memcpy(ctx_, img.data(), rgba, px * 4, 1), "download rgba8");
    if (lin) vct_device_free(ctx_, lin);
    vct_device_free(ctx_, rgba);
    if (!ok) return false;
    if (s_.present && path.size() > 4 && path.compare(path.size() - 4, 4, ".png") == 0) {
        PngImage out;
        out.width = s_.width; out.height = s_.height; out.comp = 3;
        out.data.resize(px * 3);
        for (size_t i = 0; i < px; ++i)
            for (int k = 0; k < 3; ++k) out.data[3 * i + k] = (uint8_t)(img[i] >> (8 * k));
        std::string err;
        if (!WritePng(path, out, &err)) {
            error_ = err;
            std::fprintf(stderr, "present: %s\n", err.c_str());
            return false;
        }
        return true;
    }
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "P6\n%u %u\n255\n", s_.width, s_.height);
    std::vector<unsigned char> row(s_.width * 3);
    for (uint32_t y = 0; y < s_.height; ++y) {
        for (uint32_t x = 0; x < s_.width; ++x) {               // row 0 = top (the G-buffer's ray rule)
            const uint32_t c = img[(size_t)y * s_.width + x];
            row[3 * x] = (unsigned char)(c & 255);
            row[3 * x + 1] = (unsigned char)((c >> 8) & 255);
            row[3 * x + 2] = (unsigned char)((c >> 16) & 255);
        }
        std::fwrite(row.data(), 1, row.size(), f);
    }
    std::fclose(f);
    return true;
}

bool ConeTraceRenderer::WriteVoxelView(const std::string& path, uint32_t level, uint32_t mode) {
    if (!ctx_) return false;
    const size_t px = (size_t)s_.width * s_.height;
    void* rgba = nullptr;
    if (!check(vct_device_alloc(ctx_, px * 4, &rgba), "alloc voxel view")) return false;
    std::vector<uint32_t> img(px);
    vct_voxel_view_args a{};
    a.width = s_.width; a.height = s_.height;
    a.level = level; a.mode = mode; a.shade = 1;
    a.rgba8 = (uint32_t*)rgba;
    const bool ok = check(vct_voxel_view_device(ctx_, &cam_, &a), "voxel view") &&
                    check(vct_memcpy(ctx_, img.data(), rgba, px * 4, 1), "download voxel view");
    vct_device_free(ctx_, rgba);
    if (!ok) return false;
    PngImage out;
    out.width = s_.width; out.height = s_.height; out.comp = 3;
    out.data.resize(px * 3);
    for (size_t i = 0; i < px; ++i)
        for (int k = 0; k < 3; ++k) out.data[3 * i + k] = (uint8_t)(img[i] >> (8 * k));
    std::string err;
    if (!WritePng(path, out, &err)) {
        error_ = err;
        std::fprintf(stderr, "voxel view: %s\n", err.c_str());
        return false;
    }
    return true;
}

bool ConeTraceRenderer::WriteLinear(const std::string& path) {
    if (!ctx_) return false;
    const size_t px = (size_t)s_.width * s_.height;
    void* lin = nullptr;
    if (!check(vct_device_alloc(ctx_, px * 16, &lin), "alloc linear frame")) return false;
    std::vector<float> img(px * 4);
    const bool ok = check(composite((float*)lin, nullptr), "composite") &&
                    check(vct_memcpy(ctx_, img.data(), lin, px * 16, 1), "download linear frame");
    vct_device_free(ctx_, lin);
    if (!ok) return false;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool wrote = std::fwrite(img.data(), sizeof(float), img.size(), f) == img.size();
    return std::fclose(f) == 0 && wrote;
}

}  // namespace vcthost
