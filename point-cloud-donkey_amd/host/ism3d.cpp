// ism3d.cpp — bodies of the C++ host mirror (ism3d.h). Every hot-path body is a call into libismhip.so (C ABI);
// this file only owns configuration, batching, device buffers and the training-side bookkeeping the reference does on
// the host (reference files cited per function, relative to /root/reference/src/implicit_shape_model).
#include "ism3d.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <numeric>
#include <random>

namespace ism3d {

// ---------------------------------------------------------------------------------------------------------------
// logging (reference: log4cxx macros utils/utils.h:27-38; INFO<->WARN switch implicit_shape_model.cpp:145-151)
// ---------------------------------------------------------------------------------------------------------------
static bool g_log_info = true;
#define LOG_INFO(x) do { if (g_log_info) std::cout << "INFO: " << x << std::endl; } while (0)
#define LOG_WARN(x) do { std::cout << "WARN: " << x << std::endl; } while (0)
#define LOG_ERROR(x) do { std::cerr << "ERROR: " << x << std::endl; } while (0)
void jsonWarnMissing(const std::string& name) { LOG_WARN("parameter \"" << name << "\" not found, using default"); }

// ---------------------------------------------------------------------------------------------------------------
// device plumbing
// ---------------------------------------------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    void reserve(size_t n) {
        if (n <= bytes) return;
        if (p) (void)hipFree(p);
        p = nullptr; bytes = 0;
        size_t want = n + n / 4 + 256;
        if (hipMalloc(&p, want) != hipSuccess) throw RuntimeException("hipMalloc failed");
        bytes = want;
    }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
    template <typename T> T* as() { return reinterpret_cast<T*>(p); }
    template <typename T> const T* as() const { return reinterpret_cast<const T*>(p); }
};

// the seven point arrays of a batch. The rgba buffer is reserved, passed and swapped only when the batch has colour.
struct PointArrays {
    DevBuf x, y, z, nx, ny, nz, rgba;
    std::array<DevBuf*, 6> floats() { return {{&x, &y, &z, &nx, &ny, &nz}}; }
    ismhip_point_arrays view(bool with_color) {
        return ismhip_point_arrays{x.as<float>(), y.as<float>(), z.as<float>(), nx.as<float>(), ny.as<float>(), nz.as<float>(),
                                   with_color ? rgba.as<uint32_t>() : nullptr};
    }
    void reserve(size_t n_points, bool with_color) {
        for (DevBuf* b : floats()) b->reserve(std::max<size_t>(n_points, 1) * 4);
        if (with_color) rgba.reserve(std::max<size_t>(n_points, 1) * 4);
    }
    void swap(PointArrays& o, bool with_color) {
        for (int a = 0; a < 6; ++a) floats()[a]->swap(*o.floats()[a]);
        if (with_color) rgba.swap(o.rgba);
    }
};

// owning handles of a temporary search surface / codebook (the deleter holds the context)
typedef std::unique_ptr<ismhip_cloud, std::function<void(ismhip_cloud*)>> TempCloud;
typedef std::unique_ptr<ismhip_codebook, std::function<void(ismhip_codebook*)>> TempCodebook;

struct DeviceFeatures {
    std::vector<uint32_t> off{0};     // per-object ranges of the kept features
    int dim = 0;
    uint32_t n = 0;
    DevBuf desc, lrf, kx, ky, kz, src;
};

class DeviceSession {
public:
    ismhip_ctx* ctx = nullptr;
    int n_obj = 0;
    std::vector<uint32_t> pt_off, kp_off;
    PointArrays pts, spare;               // the batch's points; spare: target of a compaction (compactPoints), swapped in afterwards
    DevBuf kx, ky, kz, krgba;
    DevBuf vox_x, vox_y, vox_z, vox_rgba, cull_pc1, cull_pc2, cull_geo, cull_col;   // VoxelGridCulling: the voxel keypoints before the culling, curvatures, scores
    DevBuf sift_curv;                     // SIFT3D: the normal curvature of every point of the batch
    float normal_radius = 0.05f;          // the model's NormalRadius (SIFT3D's curvature); set by ImplicitShapeModel::computeFeatures
    ismhip_cloud* cloud = nullptr;
    bool has_color = false;
    // vote space of the current batch (Voting::m_votes)
    DevBuf v_pos, v_w, v_cls, v_inst, v_cw, v_bs, v_bq, idx, dist;
    DevBuf v_kp, v_kpt;                   // Vote::keypoint / keypoint_training of every slot (only with Voting.RansacVoteFiltering)
    DevBuf act_off;                       // [n+1] activation ranges of the list path (ActivationStrategyThreshold)
    DevBuf obj_cen, obj_rad;              // per-object cloud centroid / farthest point (single-object max types)
    std::vector<uint32_t> slot_off;
    size_t n_slots = 0;
    int n_classes = 0;
    // scratch for raw (uncompacted) features
    DevBuf raw_lrf, raw_desc, raw_cnt;
    DevBuf raw_axis;      // SpinImage: the keypoints' looked-up normals, three runs of nkp floats
    DevBuf raw_grad;      // RIFT: the intensity gradient of every point of the batch, three floats each
    DevBuf raw_usc;       // USC: the point density of every point of the batch (uint32), then the rows' own frames, nine floats per keypoint
    DevBuf cgf_lrf, cgf_normal, cgf_rows;   // CGF: its own frames, the keypoints' PCA normals (three runs of nkp floats), a chunk of raw rows
    ismhip_mlp* cgf_mlp = nullptr;          // CGF: the embedding of cgf_mlp_file on this context
    std::string cgf_mlp_file;

    // ISMHIP_KNN_BINARY=0, read when the context is created: BSHOT codebooks keep the float search (A/B runs, tests; same answers)
    bool knn_binary_route = true;

    explicit DeviceSession(int device) {
        { const char* e = getenv("ISMHIP_KNN_BINARY"); knn_binary_route = !(e && e[0] == '0'); }
        int rc = ismhip_ctx_create(device, nullptr, &ctx);
        if (rc == ISMHIP_ERR_NODEVICE) throw RuntimeException("no gfx950 device available: the recognition path has no CPU fallback");
        if (rc != ISMHIP_OK) throw RuntimeException("ismhip_ctx_create failed");
    }
    ~DeviceSession() {
        dropCloud();
        if (cgf_mlp) ismhip_mlp_destroy(cgf_mlp);
        if (ctx) ismhip_ctx_destroy(ctx);
    }
    void check(int rc, const char* what) const {
        if (rc != ISMHIP_OK) throw RuntimeException(std::string(what) + " failed (" + std::to_string(rc) + "): " + ismhip_last_error(ctx));
    }
    void sync() const { check(ismhip_sync(ctx), "ismhip_sync"); }
    void dropCloud() { if (cloud) { ismhip_cloud_destroy(ctx, cloud); cloud = nullptr; } }
    template <typename T> static void h2d(DevBuf& b, const std::vector<T>& v) {
        b.reserve(std::max<size_t>(v.size(), 1) * sizeof(T));
        if (!v.empty() && hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) throw RuntimeException("hipMemcpy H2D failed");
    }
    template <typename T> void d2h(std::vector<T>& v, const DevBuf& b, size_t n) const {
        sync();
        v.resize(n);
        if (n && hipMemcpy(v.data(), b.p, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) throw RuntimeException("hipMemcpy D2H failed");
    }
    // the colours of a cloud or keypoint set in a coloured batch: 0 when it has none
    static void appendColors(std::vector<uint32_t>& dst, const std::vector<uint32_t>& rgba, size_t n) {
        if (rgba.size() == n) dst.insert(dst.end(), rgba.begin(), rgba.end());
        else dst.insert(dst.end(), n, 0u);
    }
    // concatenates the objects into SoA arrays and uploads them as the session's batch (pts, pt_off, n_obj, has_color); the search
    // surface of the previous batch goes first. pad_normals: a cloud without normals gets zeros, otherwise they are taken as they are.
    void uploadPoints(const std::vector<const PointCloud*>& clouds, bool with_color, bool pad_normals) {
        n_obj = (int)clouds.size();
        pt_off.assign(1, 0);
        std::vector<float> h[6]; std::vector<uint32_t> hrgba;
        for (const PointCloud* c : clouds) {
            const std::vector<float>* src[6] = {&c->x, &c->y, &c->z, &c->nx, &c->ny, &c->nz};
            const bool pad = pad_normals && !(c->nx.size() == c->size() && c->ny.size() == c->size() && c->nz.size() == c->size());
            for (int a = 0; a < 6; ++a) {
                if (a >= 3 && pad) h[a].insert(h[a].end(), c->size(), 0.f);
                else h[a].insert(h[a].end(), src[a]->begin(), src[a]->end());
            }
            if (with_color) appendColors(hrgba, c->rgba, c->size());
            pt_off.push_back((uint32_t)h[0].size());
        }
        dropCloud();
        for (int a = 0; a < 6; ++a) h2d(*pts.floats()[a], h[a]);
        has_color = with_color;
        if (with_color) h2d(pts.rgba, hrgba);
    }
    // uploads the batch and builds the search surface
    // kps == nullptr: the keypoints are computed on the device by `detector` (finishBatch)
    void uploadBatch(const std::vector<const PointCloud*>& clouds, const std::vector<KeypointSet>* kps, float cell, bool with_color, const Keypoints* detector = nullptr,
                     bool is_training = false) {
        uploadPoints(clouds, with_color, false);
        if (kps) {
            kp_off.assign(1, 0);
            std::vector<float> hkx, hky, hkz; std::vector<uint32_t> hkrgba;
            for (const KeypointSet& k : *kps) {
                hkx.insert(hkx.end(), k.x.begin(), k.x.end()); hky.insert(hky.end(), k.y.begin(), k.y.end()); hkz.insert(hkz.end(), k.z.begin(), k.z.end());
                if (with_color) appendColors(hkrgba, k.rgba, k.size());
                kp_off.push_back((uint32_t)hkx.size());
            }
            h2d(kx, hkx); h2d(ky, hky); h2d(kz, hkz);
            if (with_color) h2d(krgba, hkrgba);
        }
        finishBatch(kps ? nullptr : detector, cell, is_training);
    }
    // the point arrays of the batch are in HBM (pts, pt_off): the keypoints of a device detector (nullptr: they have been uploaded) and
    // the search surface. A voxel grid needs no surface and keeps its place in front of it; ISS3D sweeps the surface, so it comes after.
    // VoxelGridCulling does both: its voxel keypoints in front, their scores and the selection behind (is_training: DisableFilterInTraining).
    void finishBatch(const Keypoints* detector, float cell, bool is_training = false) {
        const ismhip_point_arrays p = pts.view(has_color);
        dropCloud();
        const auto* vg = dynamic_cast<const KeypointsVoxelGrid*>(detector);
        const auto* iss = dynamic_cast<const KeypointsISS3D*>(detector);
        const auto* cull = dynamic_cast<const KeypointsVoxelGridCulling*>(detector);
        const auto* sift = dynamic_cast<const KeypointsSIFT3D*>(detector);
        if (detector && !vg && !iss && !cull && !sift) throw RuntimeException("keypoint type \"" + detector->getType() + "\" has no device route");
        const size_t n_pts = pt_off.back();
        if (cull) {
            const size_t cap = std::max<size_t>(n_pts, 1) * 4;
            kx.reserve(cap); ky.reserve(cap); kz.reserve(cap);
            if (has_color) krgba.reserve(cap);
            kp_off.assign((size_t)n_obj + 1, 0);
            const bool plain = cull->isPlainVoxelGrid(is_training);
            if (!plain && cull->needsColor() && !has_color)
                throw RuntimeException("VoxelGridCulling FilterMethodColor \"colordistance\" needs clouds with colours");
            if (!plain) { vox_x.reserve(cap); vox_y.reserve(cap); vox_z.reserve(cap); if (has_color) vox_rgba.reserve(cap); }
            float* vx = plain ? kx.as<float>() : vox_x.as<float>(); float* vy = plain ? ky.as<float>() : vox_y.as<float>();
            float* vz = plain ? kz.as<float>() : vox_z.as<float>();
            uint32_t* vc = !has_color ? nullptr : (plain ? krgba.as<uint32_t>() : vox_rgba.as<uint32_t>());
            std::vector<uint32_t> vox_off((size_t)n_obj + 1, 0);
            check(ismhip_voxel_keypoints(ctx, n_obj, pt_off.data(), p.x, p.y, p.z, p.rgba, cull->getLeafSize(), (uint32_t)n_pts, vx, vy, vz, vc,
                                         plain ? kp_off.data() : vox_off.data()), "ismhip_voxel_keypoints");
            check(ismhip_cloud_create(ctx, n_obj, pt_off.data(), p.x, p.y, p.z, p.nx, p.ny, p.nz, p.rgba, cell, &cloud), "ismhip_cloud_create");
            if (plain) return;
            const size_t nkp = std::max<size_t>(vox_off.back(), 1) * 4;
            cull_geo.reserve(nkp); cull_col.reserve(nkp);
            const bool kpq = cull->geometryMethod() == ISMHIP_CULLING_GEOMETRY_KPQ;
            if (kpq) {
                cull_pc1.reserve(cap); cull_pc2.reserve(cap);
                check(ismhip_principal_curvatures(ctx, cloud, cull->getLeafSize(), cull_pc1.as<float>(), cull_pc2.as<float>(), nullptr), "ismhip_principal_curvatures");
            }
            check(ismhip_culling_scores(ctx, cloud, vox_off.data(), vx, vy, vz, vc, cull->getLeafSize(), cull->geometryMethod(), cull->colorMethod(),
                                        cull->maxSimilarColorDistance(), kpq ? cull_pc1.as<float>() : nullptr, kpq ? cull_pc2.as<float>() : nullptr,
                                        cull_geo.as<float>(), cull_col.as<float>(), nullptr), "ismhip_culling_scores");
            check(ismhip_culling_select(ctx, n_obj, vox_off.data(), cull_geo.as<float>(), cull_col.as<float>(), cull->geometryMethod() != 0, cull->colorMethod() != 0,
                                        cull->geometryType(), cull->colorType(), cull->geometryThreshold(), cull->colorThreshold(), cull->cutoffRatio(),
                                        cull->combine(), vx, vy, vz, vc, (uint32_t)n_pts, kx.as<float>(), ky.as<float>(), kz.as<float>(),
                                        has_color ? krgba.as<uint32_t>() : nullptr, nullptr, nullptr, nullptr, kp_off.data()), "ismhip_culling_select");
            return;
        }
        // SIFT3D: every point of an octave can be an extremum in every inner column, and no octave is larger than the cloud
        const size_t kp_cap = std::max<size_t>(n_pts, 1) * (sift ? (size_t)(KeypointsSIFT3D::kOctaves * KeypointsSIFT3D::kScalesPerOctave) : 1);
        if (kp_cap > 0xffffffffull) throw RuntimeException("batch too large for the keypoint arrays");
        if (detector) {
            // the keypoints stay in HBM, only the per-object counts come back
            kx.reserve(kp_cap * 4); ky.reserve(kp_cap * 4); kz.reserve(kp_cap * 4);
            if (has_color) krgba.reserve(kp_cap * 4);
            kp_off.assign((size_t)n_obj + 1, 0);
        }
        if (vg)       // KeypointsVoxelGrid::iComputeKeypoints on the device
            check(ismhip_voxel_keypoints(ctx, n_obj, pt_off.data(), p.x, p.y, p.z, p.rgba, vg->getLeafSize(), (uint32_t)n_pts, kx.as<float>(), ky.as<float>(),
                                         kz.as<float>(), has_color ? krgba.as<uint32_t>() : nullptr, kp_off.data()), "ismhip_voxel_keypoints");
        check(ismhip_cloud_create(ctx, n_obj, pt_off.data(), p.x, p.y, p.z, p.nx, p.ny, p.nz, p.rgba, cell, &cloud), "ismhip_cloud_create");
        if (iss)      // KeypointsISS3D::iComputeKeypoints on the device: points of the cloud the descriptors will see
            check(ismhip_iss3d_keypoints(ctx, cloud, (float)iss->getSalientRadius(), (float)iss->getNonMaxRadius(), iss->getGamma21(), iss->getGamma32(),
                                         iss->getMinNeighbors(), (uint32_t)n_pts, kx.as<float>(), ky.as<float>(), kz.as<float>(),
                                         has_color ? krgba.as<uint32_t>() : nullptr, nullptr, kp_off.data()), "ismhip_iss3d_keypoints");
        if (sift) {   // KeypointsSIFT3D::iComputeKeypoints on the device: the curvature of the surface at NormalRadius, then the detector
            sift_curv.reserve(std::max<size_t>(n_pts, 1) * 4);
            check(ismhip_normal_curvature(ctx, cloud, normal_radius, sift_curv.as<float>(), nullptr), "ismhip_normal_curvature");
            check(ismhip_sift3d_keypoints(ctx, cloud, sift_curv.as<float>(), sift->getRadius(), KeypointsSIFT3D::kOctaves, KeypointsSIFT3D::kScalesPerOctave,
                                          0.0f, (uint32_t)kp_cap, kx.as<float>(), ky.as<float>(), kz.as<float>(), nullptr, kp_off.data(), nullptr),
                  "ismhip_sift3d_keypoints");
            // copyPointCloud from XYZI leaves no colour (keypoints_sift3d.cpp:78)
            if (has_color && kp_off.back() > 0 && hipMemset(krgba.p, 0, (size_t)kp_off.back() * 4) != hipSuccess) throw RuntimeException("hipMemset failed");
        }
    }
    // one compaction of the batch's points: reserves the spare arrays, runs `call` (which writes them and the new offsets), makes them
    // the current ones and replaces pt_off
    void compactPoints(const char* what, const std::function<int(const ismhip_point_arrays* in, const ismhip_point_arrays* out, uint32_t* new_off)>& call) {
        spare.reserve(pt_off.back(), has_color);
        const ismhip_point_arrays in = pts.view(has_color), out = spare.view(has_color);
        std::vector<uint32_t> new_off(pt_off.size());
        check(call(&in, &out, new_off.data()), what);
        pts.swap(spare, has_color);
        pt_off = new_off;
    }
};

// ---------------------------------------------------------------------------------------------------------------
// JSONObject (utils/json_object.cpp)
// ---------------------------------------------------------------------------------------------------------------
JSONObject::JSONObject() {}
JSONObject::~JSONObject() { for (auto* p : m_params) delete p; }

Json JSONObject::configToJson() const {        // json_object.cpp:180-205
    Json object = Json::object();
    if (!getType().empty()) object["Type"] = Json::of(getType());
    Json params = Json::object();
    for (auto* p : m_params) params[p->name] = p->toJson();
    if (!params.obj.empty()) object["Parameters"] = params;
    Json children = iChildConfigsToJson();
    if (children.isObject() && !children.obj.empty()) object["Children"] = children;
    return object;
}

bool JSONObject::configFromJson(const Json& object) {   // json_object.cpp:207-240
    if (!object.isObject()) return false;
    const Json* params = object.find("Parameters");
    for (auto* p : m_params) p->fromJson(params && params->isObject() ? params->find(p->name) : nullptr);
    iPostInitConfig();
    static const Json empty = Json::object();
    const Json* children = object.find("Children");
    return iChildConfigsFromJson(children ? *children : empty);
}

static std::string dirOf(const std::string& f) { size_t p = f.find_last_of('/'); return p == std::string::npos ? std::string() : f.substr(0, p + 1); }
static std::string baseOf(const std::string& f) { size_t p = f.find_last_of('/'); return p == std::string::npos ? f : f.substr(p + 1); }

bool JSONObject::writeObject(std::string file) {
    std::string data = file;
    size_t p = data.find_last_of('.');
    if (p != std::string::npos && p > data.find_last_of('/') + 0) data = data.substr(0, p);
    return writeObject(file, data + ".ismd");
}
bool JSONObject::writeObject(std::string file, std::string fileData) {     // json_object.cpp:50-95
    Json root = Json::object();
    root["ObjectConfig"] = configToJson();
    root["ObjectData"] = Json::of(baseOf(fileData));
    std::ofstream cfg(file);
    if (!cfg) { LOG_ERROR("could not write file: " << file); return false; }
    cfg << root.dump(3) << std::endl;
    std::ofstream data(fileData, std::ios::binary);
    if (!data) { LOG_ERROR("could not write file: " << fileData); return false; }
    iSaveData(data);
    return true;
}
bool JSONObject::readObject(std::string file, bool training) {            // json_object.cpp:97-178
    std::ifstream in(file);
    if (!in) { LOG_ERROR("could not read file: " << file); return false; }
    std::stringstream ss; ss << in.rdbuf();
    Json root;
    try { root = Json::parse(ss.str()); } catch (const std::exception& e) { throw JSONException(std::string("could not parse ") + file + ": " + e.what()); }
    const Json* cfg = root.find("ObjectConfig");
    if (!cfg) throw JSONException("no ObjectConfig in " + file);
    m_input_config_file = file;
    if (!configFromJson(*cfg)) return false;
    const Json* data = root.find("ObjectData");
    if (!training && data && data->type == Json::String && !data->str.empty()) {
        std::ifstream d(dirOf(file) + data->str, std::ios::binary);
        if (!d) { LOG_ERROR("could not read data file: " << dirOf(file) + data->str); return false; }
        return iLoadData(d);
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// Keypoints: pcl::VoxelGrid centroids (keypoints/keypoints_voxel_grid.cpp:30-46). Host side:
// the step BEFORE the hot path.
// ---------------------------------------------------------------------------------------------------------------
KeypointsVoxelGrid::KeypointsVoxelGrid() { addParameter(m_leafSize, "LeafSize", 0.1f); }

KeypointSet KeypointsVoxelGrid::iComputeKeypoints(const PointCloud& c) const {
    KeypointSet out;
    const size_t n = c.size();
    if (n == 0) return out;
    float mn[3] = {c.x[0], c.y[0], c.z[0]}, mx[3] = {c.x[0], c.y[0], c.z[0]};
    for (size_t i = 0; i < n; ++i) {
        mn[0] = std::min(mn[0], c.x[i]); mx[0] = std::max(mx[0], c.x[i]);
        mn[1] = std::min(mn[1], c.y[i]); mx[1] = std::max(mx[1], c.y[i]);
        mn[2] = std::min(mn[2], c.z[i]); mx[2] = std::max(mx[2], c.z[i]);
    }
    const float inv = 1.0f / m_leafSize;
    int minb[3], divb[3];
    for (int a = 0; a < 3; ++a) { minb[a] = (int)std::floor(mn[a] * inv); divb[a] = (int)std::floor(mx[a] * inv) - minb[a] + 1; }
    const int64_t mul1 = divb[0], mul2 = (int64_t)divb[0] * divb[1];
    std::vector<std::pair<int64_t, uint32_t>> iv(n);
    for (size_t i = 0; i < n; ++i) {
        const int64_t i0 = (int64_t)(std::floor(c.x[i] * inv) - (float)minb[0]);
        const int64_t i1 = (int64_t)(std::floor(c.y[i] * inv) - (float)minb[1]);
        const int64_t i2 = (int64_t)(std::floor(c.z[i] * inv) - (float)minb[2]);
        iv[i] = {i0 + i1 * mul1 + i2 * mul2, (uint32_t)i};
    }
    std::stable_sort(iv.begin(), iv.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    const bool color = c.rgba.size() == n;
    size_t i = 0;
    while (i < n) {
        size_t j = i;
        float s[3] = {0, 0, 0}, col[3] = {0, 0, 0};
        while (j < n && iv[j].first == iv[i].first) {
            const uint32_t p = iv[j].second;
            s[0] += c.x[p]; s[1] += c.y[p]; s[2] += c.z[p];
            if (color) { col[0] += (float)((c.rgba[p] >> 16) & 0xff); col[1] += (float)((c.rgba[p] >> 8) & 0xff); col[2] += (float)(c.rgba[p] & 0xff); }
            ++j;
        }
        const float cnt = (float)(j - i);
        out.x.push_back(s[0] / cnt); out.y.push_back(s[1] / cnt); out.z.push_back(s[2] / cnt);
        if (color) out.rgba.push_back(((uint32_t)(uint8_t)(col[0] / cnt) << 16) | ((uint32_t)(uint8_t)(col[1] / cnt) << 8) | (uint32_t)(uint8_t)(col[2] / cnt));
        i = j;
    }
    return out;
}

// Keypoints: pcl::ISSKeypoint3D (keypoints/keypoints_iss3d.cpp:17-72). The detector itself is ismhip_iss3d_keypoints on the batch's search
// surface (DeviceSession::finishBatch); this class holds the configuration.
KeypointsISS3D::KeypointsISS3D() {
    addParameter(m_salientRadius, "SalientRadius", 0.1);
    addParameter(m_nonMaxRadius, "NonMaxRadius", 0.05);
    addParameter(m_gamma21, "Gamma21", 0.975);
    addParameter(m_gamma32, "Gamma32", 0.975);
    addParameter(m_minNeighbors, "MinNeighbors", 5);
}
void KeypointsISS3D::iPostInitConfig() {
    const std::pair<const char*, double> positive[] = {{"invalid ISS3D SalientRadius", m_salientRadius}, {"invalid ISS3D NonMaxRadius", m_nonMaxRadius},
                                                      {"invalid ISS3D Gamma21", m_gamma21}, {"invalid ISS3D Gamma32", m_gamma32}};
    for (const auto& p : positive)
        if (!(p.second > 0.0) || !std::isfinite(p.second) || !((float)p.second > 0.f)) throw BadParamExceptionType<double>(p.first, p.second);
    if (m_minNeighbors < 0) throw BadParamExceptionType<int>("invalid ISS3D MinNeighbors", m_minNeighbors);
}
KeypointSet KeypointsISS3D::iComputeKeypoints(const PointCloud&) const {
    throw RuntimeException("KeypointsISS3D has no host implementation: the detector runs on the device with the batch (ismhip_iss3d_keypoints)");
}

// Keypoints: pcl::SIFTKeypoint on the normals' curvature (keypoints/keypoints_sift3d.cpp:17-86). The detector itself is
// ismhip_normal_curvature + ismhip_sift3d_keypoints on the batch's search surface (DeviceSession::finishBatch); this class holds the
// configuration.
KeypointsSIFT3D::KeypointsSIFT3D() { addParameter(m_radius, "Radius", 0.05f); }
void KeypointsSIFT3D::iPostInitConfig() {
    if (!(m_radius > 0.f) || !std::isfinite(m_radius)) throw BadParamExceptionType<float>("invalid SIFT3D Radius", m_radius);
}
KeypointSet KeypointsSIFT3D::iComputeKeypoints(const PointCloud&) const {
    throw RuntimeException("KeypointsSIFT3D has no host implementation: the detector runs on the device with the batch (ismhip_sift3d_keypoints)");
}

// Keypoints: voxel-grid keypoints culled by quality scores (keypoints/keypoints_voxel_grid_culling.cpp:27-44). The detector itself is
// ismhip_voxel_keypoints + ismhip_principal_curvatures / ismhip_culling_scores / ismhip_culling_select on the batch's search surface
// (DeviceSession::finishBatch); this class holds the configuration and refuses, by name, what is not built.
KeypointsVoxelGridCulling::KeypointsVoxelGridCulling() {
    addParameter(m_leafSize, "LeafSize", 0.1f);
    addParameter(m_filter_method_geometry, "FilterMethodGeometry", std::string("None"));
    addParameter(m_filter_type_geometry, "FilterTypeGeometry", std::string("CutOff"));
    addParameter(m_filter_threshold_geometry, "FilterThresholdGeometry", 0.005f);
    addParameter(m_filter_method_color, "FilterMethodColor", std::string("None"));
    addParameter(m_filter_type_color, "FilterTypeColor", std::string("CutOff"));
    addParameter(m_filter_threshold_color, "FilterThresholdColor", 0.02f);
    addParameter(m_max_similar_color_distance, "MaxSimilarColorDistance", 0.01f);
    addParameter(m_filter_cutoff_ratio, "FilterCutoffRatio", 0.5f);
    addParameter(m_disable_filter_in_training, "DisableFilterInTraining", true);
    addParameter(m_combine_filters, "CombineFilters", std::string("RequireCombinedList"));
    addParameter(m_refine_position, "RefineKeypointPosition", false);
}
void KeypointsVoxelGridCulling::iPostInitConfig() {
    auto lower = [](std::string s) { for (char& c : s) c = (char)std::tolower((unsigned char)c); return s; };   // :62-65
    const std::string mg = lower(m_filter_method_geometry), tg = lower(m_filter_type_geometry), mc = lower(m_filter_method_color), tc = lower(m_filter_type_color);
    if (!(m_leafSize > 0.f) || !std::isfinite(m_leafSize)) throw BadParamExceptionType<float>("invalid VoxelGridCulling LeafSize: the voxel edge and ball radius must be positive", m_leafSize);
    if (mg == "gaussian")
        throw BadParamExceptionType<std::string>("VoxelGridCulling FilterMethodGeometry \"gaussian\" is not built: PCL takes the query's normal from the surface "
                                                 "normals at the keypoint's index, an unrelated point since keypoints are not surface points, so the reference's "
                                                 "result is noise (built: none, curvature, kpq)", m_filter_method_geometry);
    if (mg == "none") m_geometry = ISMHIP_CULLING_GEOMETRY_NONE;
    else if (mg == "curvature") m_geometry = ISMHIP_CULLING_GEOMETRY_CURVATURE;
    else if (mg == "kpq") m_geometry = ISMHIP_CULLING_GEOMETRY_KPQ;
    else throw BadParamExceptionType<std::string>("unsupported VoxelGridCulling FilterMethodGeometry (built: none, curvature, kpq)", m_filter_method_geometry);
    if (tg == "auto")
        throw BadParamExceptionType<std::string>("VoxelGridCulling FilterTypeGeometry \"auto\" is not built: the source marks it experimental and it is undefined "
                                                 "for a zero histogram step (built: cutoff, threshold)", m_filter_type_geometry);
    if (tg == "cutoff") m_geometry_type = ISMHIP_CULLING_TYPE_CUTOFF;
    else if (tg == "threshold") m_geometry_type = ISMHIP_CULLING_TYPE_THRESHOLD;
    else throw BadParamExceptionType<std::string>("unsupported VoxelGridCulling FilterTypeGeometry (built: cutoff, threshold)", m_filter_type_geometry);
    if (mc == "none") m_color = ISMHIP_CULLING_COLOR_NONE;
    else if (mc == "colordistance") m_color = ISMHIP_CULLING_COLOR_DISTANCE;
    else throw BadParamExceptionType<std::string>("unsupported VoxelGridCulling FilterMethodColor (built: none, colordistance)", m_filter_method_color);
    if (tc == "cutoff") m_color_type = ISMHIP_CULLING_TYPE_CUTOFF;
    else if (tc == "threshold") m_color_type = ISMHIP_CULLING_TYPE_THRESHOLD;
    else throw BadParamExceptionType<std::string>("unsupported VoxelGridCulling FilterTypeColor (built: cutoff, threshold)", m_filter_type_color);
    if (m_refine_position) throw BadParamException("VoxelGridCulling RefineKeypointPosition is not built: position refinement is a later change");
    if (!(m_filter_cutoff_ratio >= 0.f && m_filter_cutoff_ratio < 1.f))
        throw BadParamExceptionType<float>("invalid VoxelGridCulling FilterCutoffRatio: the share of keypoints to omit must lie in [0, 1)", m_filter_cutoff_ratio);
    if (m_combine_filters == "RequireOne") m_combine = ISMHIP_CULLING_REQUIRE_ONE;          // case-sensitive, as :240-251 compares
    else if (m_combine_filters == "RequireBoth") m_combine = ISMHIP_CULLING_REQUIRE_BOTH;
    else if (m_combine_filters == "RequireCombinedList") m_combine = ISMHIP_CULLING_REQUIRE_COMBINED_LIST;
    else throw BadParamExceptionType<std::string>("unknown VoxelGridCulling CombineFilters: the reference silently drops every keypoint "
                                                  "(one of RequireOne, RequireBoth, RequireCombinedList)", m_combine_filters);
}
KeypointSet KeypointsVoxelGridCulling::iComputeKeypoints(const PointCloud&) const {
    throw RuntimeException("KeypointsVoxelGridCulling has no host implementation: the detector runs on the device with the batch "
                           "(ismhip_voxel_keypoints, ismhip_culling_scores, ismhip_culling_select)");
}

// ---------------------------------------------------------------------------------------------------------------
// Features (features/features.cpp)
// ---------------------------------------------------------------------------------------------------------------
Features::Features() : m_numThreads(0) {
    addParameter(m_referenceFrameRadius, "ReferenceFrameRadius", 0.2f);
    addParameter(m_referenceFrameType, "ReferenceFrameType", std::string("SHOT"));
}

void Features::checkReferenceFrameType() const {   // features.cpp:153-179
    if (m_referenceFrameType == "SHOT" || m_referenceFrameType == "SHOTNA") return;
    if (m_referenceFrameType == "BOARD" || m_referenceFrameType == "FLARE")
        throw RuntimeException("reference frame type \"" + m_referenceFrameType + "\" is not built on the MI355X path (built: \"SHOT\", \"SHOTNA\")");
    throw BadParamExceptionType<std::string>("invalid reference frame type", m_referenceFrameType);   // features.cpp:178
}

std::shared_ptr<DeviceFeatures> Features::operator()(DeviceSession& s) const {   // features.cpp:40-116
    checkReferenceFrameType();
    const bool shotna = m_referenceFrameType == "SHOTNA";   // features.cpp:153-179: the z sign voted by the cloud's normals
    const uint32_t nkp = s.kp_off.back();
    const int D = getDescriptorLength();
    auto f = std::make_shared<DeviceFeatures>();
    f->dim = D;
    f->off.assign(s.n_obj + 1, 0);
    if (nkp == 0) return f;
    LOG_INFO("computing reference frames");
    s.raw_lrf.reserve((size_t)nkp * 9 * 4); s.raw_desc.reserve((size_t)nkp * D * 4); s.raw_cnt.reserve((size_t)nkp * 4);
    s.check((shotna ? ismhip_shotna_lrf : ismhip_shot_lrf)(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(),
                                                           m_referenceFrameRadius, s.raw_lrf.as<float>()),
            shotna ? "ismhip_shotna_lrf" : "ismhip_shot_lrf");
    LOG_INFO("computing descriptors at keypoint positions");
    iComputeDescriptors(s, s.raw_lrf.as<float>(), s.raw_desc.as<float>(), s.raw_cnt.as<uint32_t>());
    // invalid frames and NaN descriptors are dropped, order preserved (features.cpp:66-76, implicit_shape_model.cpp:1276-1308)
    f->desc.reserve((size_t)nkp * D * 4); f->lrf.reserve((size_t)nkp * 9 * 4);
    f->kx.reserve((size_t)nkp * 4); f->ky.reserve((size_t)nkp * 4); f->kz.reserve((size_t)nkp * 4); f->src.reserve((size_t)nkp * 4);
    int all_kept = 0;
    s.check(ismhip_compact_descriptor_rows(s.ctx, s.n_obj, s.kp_off.data(), D, s.raw_desc.as<float>(), s.raw_lrf.as<float>(), s.kx.as<float>(),
                                           s.ky.as<float>(), s.kz.as<float>(), f->desc.as<float>(), f->lrf.as<float>(), f->kx.as<float>(),
                                           f->ky.as<float>(), f->kz.as<float>(), f->src.as<uint32_t>(), f->off.data(), &all_kept),
            "ismhip_compact_descriptor_rows");
    if (all_kept) {
        // nothing was dropped and nothing was copied: the raw matrices become the features, the keypoints are duplicated (12 bytes each)
        f->desc.swap(s.raw_desc); f->lrf.swap(s.raw_lrf);
        s.sync();
        if (nkp && (hipMemcpy(f->kx.p, s.kx.p, (size_t)nkp * 4, hipMemcpyDeviceToDevice) != hipSuccess ||
                    hipMemcpy(f->ky.p, s.ky.p, (size_t)nkp * 4, hipMemcpyDeviceToDevice) != hipSuccess ||
                    hipMemcpy(f->kz.p, s.kz.p, (size_t)nkp * 4, hipMemcpyDeviceToDevice) != hipSuccess))
            throw RuntimeException("hipMemcpy D2D failed");
    }
    f->n = f->off.back();
    if (f->n < nkp) LOG_WARN("discarded " << (nkp - f->n) << " keypoint(s) with invalid reference frame or NaN descriptor");
    LOG_INFO("obtained " << f->n << " " << getType() << " descriptors");
    return f;
}

FeaturesSHOT::FeaturesSHOT() { addParameter(m_radius, "Radius", 0.1f); }
FeaturesCSHOT::FeaturesCSHOT() { addParameter(m_radius, "Radius", 0.1f); }
FeaturesFPFH::FeaturesFPFH() { addParameter(m_radius, "Radius", 0.1f); }
FeaturesBSHOT::FeaturesBSHOT() { addParameter(m_radius, "Radius", 0.1f); }       // features_bshot.cpp:31-34
FeaturesSHORTSHOT::FeaturesSHORTSHOT() {         // features_short_shot.cpp:21-32
    addParameter(m_radius, "Radius", 0.1f);
    addParameter(m_use_min_radius, "UseMinRadius", false);
    addParameter(m_min_radius_relative, "ShortShotMinRadius", 0.0);
    addParameter(m_feature_dims, "ShortShotDims", 32);
    addParameter(m_log_radius, "ShortShotLogRadius", false);
    addParameter(m_r_bins, "ShortShotRBins", 2);
    addParameter(m_e_bins, "ShortShotEBins", 2);
    addParameter(m_a_bins, "ShortShotABins", 8);
    addParameter(m_bin_type, "ShortShotBinType", std::string("auto"));
}
float FeaturesSHORTSHOT::getMinRadius() const {  // :88-103 (the reference's default relative value is the float 0.1f)
    if (m_use_min_radius) return (float)((double)m_radius * m_min_radius_relative);
    return m_log_radius ? (float)((double)m_radius * (double)0.1f) : 0.0f;
}
void FeaturesSHORTSHOT::iPostInitConfig() {      // configureSphericalGrid, :285-366: run once the config has been read
    Features::iPostInitConfig();
    static const int sizes[9][4] = {{8, 1, 1, 8}, {16, 2, 2, 4}, {24, 2, 2, 6}, {32, 2, 2, 8}, {64, 2, 4, 8}, {96, 3, 4, 8}, {128, 4, 4, 8}, {192, 6, 4, 8}, {256, 8, 4, 8}};
    bool fallback = false;
    if (m_bin_type == "auto") {
        const int* row = nullptr;
        for (const auto& r : sizes) if (r[0] == m_feature_dims) row = r;
        if (row) { m_r_bins = row[1]; m_e_bins = row[2]; m_a_bins = row[3]; }
        else { LOG_ERROR("Unsupported Short SHOT dimensions for automatic bin configuration: " << m_feature_dims << "! Setting to 32 dimensions with default bins."); fallback = true; }
    } else if (m_bin_type == "manual") {
        if (m_r_bins < 1 || m_e_bins < 1 || m_a_bins < 1) throw RuntimeException(getType() + ": fewer than one bin on an axis");
        if ((long long)m_r_bins * m_e_bins * m_a_bins > ISMHIP_SHORT_SHOT_MAX_DIM)
            throw RuntimeException(getType() + ": more than " + std::to_string(ISMHIP_SHORT_SHOT_MAX_DIM) + " bins are not built on the MI355X path");
        m_feature_dims = m_r_bins * m_e_bins * m_a_bins;
    } else {
        LOG_ERROR("Unsupported Short SHOT bins configuration type: " << m_bin_type << "! Setting to 32 dimensions with default bins.");
        fallback = true;
    }
    if (fallback) { m_r_bins = 2; m_e_bins = 2; m_a_bins = 8; m_feature_dims = 32; }
    const float mr = getMinRadius();
    if (!(mr >= 0.0f)) throw RuntimeException(getType() + ": negative minimum radius");
    // the reference divides by log(Radius / min_radius) (0 for min_radius == 0) and converts the NaN to int: refused, never altered
    if (m_log_radius && !(mr > 0.0f && mr < m_radius))
        throw RuntimeException(getType() + ": ShortShotLogRadius needs a minimum radius inside (0, Radius); UseMinRadius with ShortShotMinRadius 0 leaves none");
}
FeaturesSHORTCSHOT::FeaturesSHORTCSHOT() {       // features_short_cshot.cpp:21-33: the nine of FeaturesSHORTSHOT and
    addParameter(m_color_feature_dims, "ShortColorShotDims", 32);
    addParameter(m_color_hist_size, "ShortColorShotHistSize", 15);
}
void FeaturesSHORTCSHOT::checkInput(const PointCloud& cloud) const {
    if (!cloud.empty() && cloud.rgba.size() != cloud.size()) throw RuntimeException("SHORT_CSHOT needs coloured point clouds");
}
void FeaturesSHORTCSHOT::iPostInitConfig() {     // configureSphericalGrid, then configureSphericalColorGrid (:592-646): automatic sizes only
    FeaturesSHORTSHOT::iPostInitConfig();
    static const int sizes[7][4] = {{8, 1, 1, 8}, {16, 2, 2, 4}, {24, 2, 2, 6}, {32, 2, 2, 8}, {64, 2, 4, 8}, {96, 3, 4, 8}, {128, 4, 4, 8}};
    const int* row = nullptr;
    for (const auto& r : sizes) if (r[0] == m_color_feature_dims) row = r;
    if (row) { m_r_color_bins = row[1]; m_e_color_bins = row[2]; m_a_color_bins = row[3]; }
    else {
        LOG_ERROR("Unsupported Short Color SHOT dimensions for bin configuration: " << m_color_feature_dims << "! Setting to 32 dimensions.");
        m_r_color_bins = 2; m_e_color_bins = 2; m_a_color_bins = 8; m_color_feature_dims = 32;
    }
    if (m_color_hist_size < 1) throw RuntimeException("SHORT_CSHOT: ShortColorShotHistSize below 1");
    if ((long long)m_feature_dims + (long long)m_color_feature_dims * m_color_hist_size > ISMHIP_SHORT_CSHOT_MAX_DIM)
        throw RuntimeException("SHORT_CSHOT: a descriptor longer than " + std::to_string(ISMHIP_SHORT_CSHOT_MAX_DIM) + " is not built on the MI355X path");
}
FeaturesCospair::FeaturesCospair() { addParameter(m_radius, "Radius", 0.1f); }   // features_cospair.cpp:19-22
FeaturesSpinImage::FeaturesSpinImage() { addParameter(m_radius, "Radius", 0.1f); }   // features_spin_image.cpp:19-22
FeaturesRSD::FeaturesRSD() {                     // features_rsd.cpp:19-23
    addParameter(m_radius, "Radius", 0.1f);
    addParameter(m_use_hist, "UseFullRSDHistogram", true);
}
FeaturesRIFT::FeaturesRIFT() { addParameter(m_radius, "Radius", 0.1f); }   // features_rift.cpp:20-23
FeaturesESFLocal::FeaturesESFLocal() { addParameter(m_radius, "Radius", 0.1f); }   // features_esf_local.cpp:21
FeaturesUSC::FeaturesUSC() { addParameter(m_radius, "Radius", 0.1f); }             // features_usc.cpp:20-23
FeaturesCGF::FeaturesCGF() {                     // features_cgf.cpp:22-25
    addParameter(m_radius, "Radius", 0.1f);
    addParameter(m_model_file, "CgfModelFile", std::string("embed_model_910000.cgfw"));
}
FeaturesCGF::~FeaturesCGF() { if (m_weights) ismhip_cgfw_close(m_weights); }
void FeaturesCGF::iPostInitConfig() {
    Features::iPostInitConfig();
    if (m_weights) { ismhip_cgfw_close(m_weights); m_weights = nullptr; m_dim = 0; }
    char err[512] = "";
    if (ismhip_cgfw_open(m_model_file.c_str(), ISMHIP_CGF_RAW_DIM, &m_weights, err, (int)sizeof(err)) != ISMHIP_OK)
        throw RuntimeException(std::string("CGF: CgfModelFile: ") + err);
    int out = 0;
    ismhip_cgfw_layer(m_weights, ismhip_cgfw_layers(m_weights) - 1, nullptr, &out, nullptr, nullptr, nullptr);
    m_dim = out;
}
void FeaturesCospair::checkInput(const PointCloud& cloud) const {
    if (!cloud.empty() && cloud.rgba.size() != cloud.size()) throw RuntimeException("CoSPAIR needs coloured point clouds");
}
void FeaturesRIFT::checkInput(const PointCloud& cloud) const {
    if (!cloud.empty() && cloud.rgba.size() != cloud.size()) throw RuntimeException("RIFT needs coloured point clouds");
}

void FeaturesSHOT::iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const {   // features_shot.cpp:28-81
    s.check(ismhip_shot352(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), lrf9, m_radius, desc_out, counts_out),
            "ismhip_shot352");
}
void FeaturesBSHOT::iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const {  // features_bshot.cpp:40-107
    s.check(ismhip_bshot352(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), lrf9, m_radius, desc_out, counts_out),
            "ismhip_bshot352");
}
void FeaturesCSHOT::iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const {  // features_cshot.cpp:28-103
    if (!s.has_color) throw RuntimeException("CSHOT needs coloured point clouds");
    s.check(ismhip_cshot1344(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), s.krgba.as<uint32_t>(), lrf9,
                             m_radius, desc_out, counts_out), "ismhip_cshot1344");
}
void FeaturesFPFH::iComputeDescriptors(DeviceSession& s, const float*, float* desc_out, uint32_t* counts_out) const {        // features_fpfh.cpp:27-72
    s.check(ismhip_fpfh33(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), m_radius, desc_out, counts_out),
            "ismhip_fpfh33");
}
void FeaturesSHORTSHOT::iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const {   // features_short_shot.cpp:38-156
    s.check(ismhip_short_shot(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), lrf9, m_radius, getMinRadius(),
                              m_log_radius ? 1 : 0, m_r_bins, m_e_bins, m_a_bins, desc_out, counts_out), "ismhip_short_shot");
}
void FeaturesSHORTCSHOT::iComputeDescriptors(DeviceSession& s, const float* lrf9, float* desc_out, uint32_t* counts_out) const {   // features_short_cshot.cpp:62-223
    if (!s.has_color) throw RuntimeException("SHORT_CSHOT needs coloured point clouds");
    s.check(ismhip_short_cshot(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), s.krgba.as<uint32_t>(), lrf9, m_radius,
                               getMinRadius(), m_log_radius ? 1 : 0, m_r_bins, m_e_bins, m_a_bins, m_r_color_bins, m_e_color_bins, m_a_color_bins,
                               m_color_hist_size, desc_out, counts_out), "ismhip_short_cshot");
}
void FeaturesCospair::iComputeDescriptors(DeviceSession& s, const float*, float* desc_out, uint32_t* counts_out) const {     // features_cospair.cpp:28-77
    if (!s.has_color) throw RuntimeException("CoSPAIR needs coloured point clouds");
    s.check(ismhip_cospair(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), m_radius, desc_out, counts_out,
                           nullptr, nullptr), "ismhip_cospair");
}
// features_spin_image.cpp:28-87: the keypoints' normals by coordinate equality (:36-53), then the spin images about them (:61-69)
void FeaturesSpinImage::iComputeDescriptors(DeviceSession& s, const float*, float* desc_out, uint32_t* counts_out) const {
    const size_t nkp = s.kp_off.back();
    s.raw_axis.reserve(nkp * 3 * 4);
    float *ax = s.raw_axis.as<float>(), *ay = ax + nkp, *az = ay + nkp;
    s.check(ismhip_keypoint_normals(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), ax, ay, az, nullptr),
            "ismhip_keypoint_normals");
    s.check(ismhip_spin_image(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), ax, ay, az, m_radius,
                              ISMHIP_SPIN_IMAGE_WIDTH, desc_out, counts_out), "ismhip_spin_image");
}
// features_rsd.cpp:29-103: search radius and plane radius are both Radius (:49-51); the histogram is normalised (:99-100), the radii are not
void FeaturesRSD::iComputeDescriptors(DeviceSession& s, const float*, float* desc_out, uint32_t* counts_out) const {
    s.check(ismhip_rsd(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), m_radius, m_use_hist ? 1 : 0, desc_out,
                       counts_out), "ismhip_rsd");
}
// features_rift.cpp:29-96: the intensity gradients of the whole cloud (:53-62), then the 8 x 16 RIFT rows of the keypoints (:66-78)
void FeaturesRIFT::iComputeDescriptors(DeviceSession& s, const float*, float* desc_out, uint32_t* counts_out) const {
    if (!s.has_color) throw RuntimeException("RIFT needs coloured point clouds");
    s.raw_grad.reserve(std::max<size_t>(s.pt_off.back(), 1) * 3 * 4);
    s.check(ismhip_intensity_gradients(s.ctx, s.cloud, m_radius, s.raw_grad.as<float>(), nullptr), "ismhip_intensity_gradients");
    s.check(ismhip_rift(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), m_radius, ISMHIP_RIFT_DISTANCE_BINS,
                        ISMHIP_RIFT_GRADIENT_BINS, s.raw_grad.as<float>(), desc_out, counts_out), "ismhip_rift");
}
// features_esf_local.cpp: PCL's ESFEstimation per keypoint ball; the sample count and the seed of the draws are the library's constants
void FeaturesESFLocal::iComputeDescriptors(DeviceSession& s, const float*, float* desc_out, uint32_t* counts_out) const {
    s.check(ismhip_esf_local(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), m_radius, ISMHIP_ESF_SAMPLES,
                             ISMHIP_ESF_SEED, desc_out, counts_out, nullptr, nullptr), "ismhip_esf_local");
}
// features_usc.cpp:28-75: the density of the cloud's points once, PCL's own frames (SHOT frames at Radius - 0.1, :52-54; lrf9, the frames
// of ReferenceFrameType, only decided which keypoints stay), then the rows with the minimal radius Radius / 10 (:50)
void FeaturesUSC::iComputeDescriptors(DeviceSession& s, const float*, float* desc_out, uint32_t* counts_out) const {
    const size_t n_pts = std::max<size_t>(s.pt_off.back(), 1), nkp = s.kp_off.back();
    s.raw_usc.reserve(n_pts * 4 + nkp * 9 * 4);
    uint32_t* density = s.raw_usc.as<uint32_t>();
    float* frames = (float*)(density + n_pts);
    s.check(ismhip_point_density(s.ctx, s.cloud, USC_POINT_DENSITY_RADIUS, density), "ismhip_point_density");
    const float frame_radius = m_radius <= 0.1f ? 0.1f : m_radius - 0.1f;
    s.check(ismhip_shot_lrf(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), frame_radius, frames), "ismhip_shot_lrf");
    s.check(ismhip_usc(s.ctx, s.cloud, s.kp_off.data(), s.kx.as<float>(), s.ky.as<float>(), s.kz.as<float>(), frames, m_radius, m_radius / 10.0f, density,
                       desc_out, counts_out, nullptr), "ismhip_usc");
}

// features_cgf.cpp:46-68 -> cgf.cpp:64-165 and embedding.py: the three lengths after their trip through std::to_string, CGF's own frames and
// keypoint normals, then raw rows and embedding in chunks of keypoints (262 144 raw rows would be 2.35 GB; the chunk size does not show)
void FeaturesCGF::iComputeDescriptors(DeviceSession& s, const float*, float* desc_out, uint32_t* counts_out) const {
    if (!m_weights) throw RuntimeException("CGF: no weights loaded (CgfModelFile)");
    if (!s.cgf_mlp || s.cgf_mlp_file != m_model_file) {
        if (s.cgf_mlp) { ismhip_mlp_destroy(s.cgf_mlp); s.cgf_mlp = nullptr; }
        s.check(ismhip_mlp_from_cgfw(s.ctx, m_weights, &s.cgf_mlp), "ismhip_mlp_from_cgfw");
        s.cgf_mlp_file = m_model_file;
    }
    auto rounded = [](double v) { char b[64]; snprintf(b, sizeof(b), "%f", v); return strtod(b, nullptr); };   // std::to_string, std::stod
    const double R = rounded((double)m_radius), rmin = rounded(m_radius * 0.05), rl = rounded(m_radius * 0.75);
    const uint32_t nkp = s.kp_off.back();
    const float *kx = s.kx.as<float>(), *ky = s.ky.as<float>(), *kz = s.kz.as<float>();
    s.cgf_lrf.reserve((size_t)nkp * 9 * 4); s.cgf_normal.reserve((size_t)nkp * 3 * 4);
    float* nrm = s.cgf_normal.as<float>();
    s.check(ismhip_shot_lrf(s.ctx, s.cloud, s.kp_off.data(), kx, ky, kz, (float)rl, s.cgf_lrf.as<float>()), "ismhip_shot_lrf");
    s.check(ismhip_keypoint_normals_pca(s.ctx, s.cloud, s.kp_off.data(), kx, ky, kz, (float)(0.1 * R), nrm, nrm + nkp, nrm + 2 * (size_t)nkp),
            "ismhip_keypoint_normals_pca");
    uint32_t chunk = 32768;
    if (const char* e = getenv("ISMHIP_CGF_CHUNK")) { const long v = atol(e); if (v > 0) chunk = (uint32_t)v; }   // tests: the result must not move
    s.cgf_rows.reserve((size_t)std::min(chunk, nkp) * ISMHIP_CGF_RAW_DIM * 4);
    std::vector<uint32_t> sub(s.kp_off.size());
    for (uint32_t b = 0; b < nkp; b += chunk) {
        const uint32_t e = std::min(nkp, b + chunk);
        for (size_t o = 0; o < sub.size(); ++o) sub[o] = std::min(std::max(s.kp_off[o], b), e) - b;   // the keypoints [b, e) of every object
        s.check(ismhip_cgf_raw(s.ctx, s.cloud, sub.data(), kx + b, ky + b, kz + b, s.cgf_lrf.as<float>() + (size_t)b * 9, nrm + b, nrm + nkp + b,
                               nrm + 2 * (size_t)nkp + b, R, rmin, s.cgf_rows.as<float>(), counts_out + b), "ismhip_cgf_raw");
        s.check(ismhip_mlp_forward(s.ctx, s.cgf_mlp, s.cgf_rows.as<float>(), e - b, desc_out + (size_t)b * m_dim), "ismhip_mlp_forward");
    }
}

// ---------------------------------------------------------------------------------------------------------------
// activation strategy + codebook
// ---------------------------------------------------------------------------------------------------------------
ActivationStrategy::ActivationStrategy() {       // activation_strategy.cpp:16-22
    addParameter(m_use_distance_ratio, "UseDistanceRatio", false);
    addParameter(m_distance_ratio_threshold, "DistanceRatioThreshold", 0.95f);
}
ActivationStrategyKNN::ActivationStrategyKNN() { addParameter(m_k, "K", 1); }   // activation_strategy_knn.cpp:19

Codebook::Codebook() {                           // codebook.cpp:28-41
    m_activationStrategy.reset(new ActivationStrategyKNN());
    addParameter(m_useClassWeight, "UseClassWeight", false);
    addParameter(m_useVoteWeight, "UseVoteWeight", false);
    addParameter(m_useMatchingWeight, "UseMatchingWeight", false);
    addParameter(m_useCodewordWeight, "UseCodewordWeight", false);
    addParameter(m_use_partial_shot, "UsePartialShot", false);
    addParameter(m_partial_shot_type, "PartialShotType", std::string("front"));
    addParameter(m_use_random_codebook, "UseRandomCodebook", false);
    addParameter(m_random_codebook_factor, "RandomCodebookFactor", 1.0f);
}
Codebook::~Codebook() {
    if (m_dev && m_dev_session) ismhip_codebook_destroy(m_dev_session->ctx, m_dev);
}
Json Codebook::iChildConfigsToJson() const {
    Json c = Json::object();
    if (m_activationStrategy) c["ActivationStrategy"] = m_activationStrategy->configToJson();
    return c;
}
bool Codebook::iChildConfigsFromJson(const Json& c) {
    if (const Json* a = c.find("ActivationStrategy")) m_activationStrategy.reset(Factory<ActivationStrategy>::create(*a));
    return m_activationStrategy != nullptr;
}

// Codebook::getSignatureMask (codebook.cpp:952-1036) -> kept descriptor columns of SHOT-352 (11 per signature)
static std::vector<int32_t> partialShotColumns(const std::string& type) {
    std::vector<bool> m(32, false);
    auto rng = [&](int a, int b) { for (int i = a; i <= b; ++i) m[i] = true; };
    if (type == "front" || type == "dense_x") rng(8, 23);
    else if (type == "back" || type == "sparse_x") { rng(0, 7); rng(24, 31); }
    else if (type == "left" || type == "positive_y") rng(16, 31);
    else if (type == "right" || type == "negative_y") rng(0, 15);
    else if (type == "top" || type == "dense_z") { for (int i = 1; i < 32; i += 2) m[i] = true; }
    else if (type == "bottom" || type == "sparse_z") { for (int i = 0; i < 32; i += 2) m[i] = true; }
    else if (type == "dense_x_or_z") { rng(8, 23); for (int i = 1; i < 32; i += 2) m[i] = true; }
    else if (type == "dense_x_and_z") { for (int i = 9; i <= 23; i += 2) m[i] = true; }
    else if (type == "front_turn_left") rng(12, 27);
    else if (type == "front_turn_right") rng(4, 19);
    else { LOG_WARN("Unknown partial shot type: " << type << "! Using complete descriptor!"); m.assign(32, true); }
    std::vector<int32_t> cols;
    for (int sidx = 0; sidx < 32; ++sidx) if (m[sidx]) for (int j = 0; j < 11; ++j) cols.push_back(sidx * 11 + j);
    return cols;
}

void Codebook::upload(DeviceSession& s) const {
    if (!m_dirty && m_dev && m_dev_session == &s) return;
    if (m_dev && m_dev_session) ismhip_codebook_destroy(m_dev_session->ctx, m_dev);
    m_dev = nullptr; m_dev_session = &s;
    const CodebookData& d = m_data;
    if (d.numWords() == 0) return;
    std::vector<float> partial;
    const float* words = d.words.data(); int dim = d.dim;
    if (m_use_partial_shot) {
        // iLoadData builds the partial codewords (codebook.cpp:862-930). Plain SHOT only: with CSHOT the reference's loop leaks hist_size = 31
        // into the shape part of every feature after the first and produces descriptors of unequal length (:419, :458).
        if (d.dim != ISMHIP_SHOT_DIM) throw RuntimeException("UsePartialShot is built for SHOT-352 codebooks only");
        m_partial_cols = partialShotColumns(m_partial_shot_type);
        dim = (int)m_partial_cols.size();
        partial.resize((size_t)d.numWords() * dim);
        for (int w = 0; w < d.numWords(); ++w) for (int c = 0; c < dim; ++c) partial[(size_t)w * dim + c] = d.words[(size_t)w * d.dim + m_partial_cols[c]];
        words = partial.data();
    } else m_partial_cols.clear();
    s.check(ismhip_codebook_create(s.ctx, d.numWords(), dim, words, d.word_weight.empty() ? nullptr : d.word_weight.data(),
                                   d.vote_offsets.data(), d.vote_xyz.data(), d.vote_weight.empty() ? nullptr : d.vote_weight.data(),
                                   d.vote_class_weight.empty() ? nullptr : d.vote_class_weight.data(), d.vote_class.data(), d.vote_instance.data(),
                                   d.vote_bbox_quat.empty() ? nullptr : d.vote_bbox_quat.data(), d.vote_bbox_size.empty() ? nullptr : d.vote_bbox_size.data(),
                                   (int)d.class_sigma.size(), d.class_sigma.data(), &m_dev), "ismhip_codebook_create");
    if ((int)d.word_class.size() == d.numWords()) s.check(ismhip_codebook_set_word_class(s.ctx, m_dev, d.word_class.data()), "ismhip_codebook_set_word_class");
    if (d.word_keypoint.size() == (size_t)d.numWords() * 3)       // Codeword::getFeaturePosition: Vote::keypoint_training (voting.cpp:71)
        s.check(ismhip_codebook_set_word_keypoint(s.ctx, m_dev, d.word_keypoint.data()), "ismhip_codebook_set_word_keypoint");
    if (m_binary_words && s.knn_binary_route) {
        // BSHOT codewords are zeros and ones unless a k-means clustering averaged them (ISMHIP_ERR_INVALID) or the codebook outgrows the
        // 32-bit key (ISMHIP_ERR_UNSUPPORTED): those keep the float search, which gives the same exact answers
        const int rc = ismhip_codebook_make_binary(s.ctx, m_dev);
        if (rc != ISMHIP_OK && rc != ISMHIP_ERR_INVALID && rc != ISMHIP_ERR_UNSUPPORTED) s.check(rc, "ismhip_codebook_make_binary");
    }
    m_dirty = false;
}

// the metrics whose BSHOT searches take ismhip_knn_binary (bit ISMHIP_METRIC_*): those for which its slowest repetition beat the float
// route's fastest (tools/bshot_time.py)
static const unsigned KNN_BINARY_ROUTE_METRICS = (1u << ISMHIP_METRIC_L2SQ) | (1u << ISMHIP_METRIC_CHI2);
int ActivationStrategyKNN::activateKNN(DeviceSession& s, const ismhip_codebook* codewords, const DeviceFeatures& f, int metric,
                                       int32_t* idx_out, float* dist_out, const float* desc) const {     // activation_strategy_knn.h:41-126
    if (m_k > ISMHIP_KNN_LARGE_K_MAX) throw RuntimeException("KNN activation with K > 1024 (ISMHIP_KNN_LARGE_K_MAX) is not built");
    if (f.n == 0) return m_k;
    if (!desc) desc = f.desc.as<float>();                        // desc: the (possibly partial, codebook.cpp:416-475) descriptors to match
    if (m_use_distance_ratio && m_is_detection && m_k == 1)     // the reference applies the ratio only for K == 1
        s.check(ismhip_knn_ratio(s.ctx, codewords, metric, (int)f.n, desc, m_distance_ratio_threshold, idx_out, dist_out), "ismhip_knn_ratio");
    else if (m_k > 16)
        s.check(ismhip_knn_large_k(s.ctx, codewords, metric, (int)f.n, desc, m_k, idx_out, dist_out), "ismhip_knn_large_k");
    else if (ismhip_codebook_has_binary(codewords) == 1 && (KNN_BINARY_ROUTE_METRICS >> metric & 1))
        // a speed route like the library's own gates: both functors are the Hamming distance on 0/1 rows, the answers are bit-identical
        s.check(ismhip_knn_binary(s.ctx, codewords, (int)f.n, desc, m_k, idx_out, dist_out), "ismhip_knn_binary");
    else
        s.check(ismhip_knn(s.ctx, codewords, metric, (int)f.n, desc, m_k, idx_out, dist_out), "ismhip_knn");
    return m_k;
}

ActivationStrategyKnnRule::ActivationStrategyKnnRule() { addParameter(m_k, "K", 3); m_is_detection = false; m_k = 3; }   // activation_strategy_knn_rule.cpp:16-22
int ActivationStrategyKnnRule::activateKNN(DeviceSession& s, const ismhip_codebook* codewords, const DeviceFeatures& f, int metric,
                                           int32_t* idx_out, float* dist_out, const float* desc) const {
    if (f.n == 0) return 1;
    if (!desc) desc = f.desc.as<float>();
    if (!m_is_detection) s.check(ismhip_knn(s.ctx, codewords, metric, (int)f.n, desc, 1, idx_out, dist_out), "ismhip_knn");
    else s.check(ismhip_knn_rule(s.ctx, codewords, metric, (int)f.n, desc, m_distance_ratio_threshold, idx_out, dist_out), "ismhip_knn_rule");
    return 1;
}

ActivationStrategyThreshold::ActivationStrategyThreshold() { addParameter(m_threshold, "Threshold", 1.0f); }   // activation_strategy_threshold.cpp:20
int ActivationStrategyThreshold::activateKNN(DeviceSession&, const ismhip_codebook*, const DeviceFeatures&, int, int32_t*, float*, const float*) const {
    throw RuntimeException("Threshold activation has no fixed number of activations per feature: use the list path");
}

// ActivationStrategyThreshold over n descriptors (device, n x dim): act_off [n+1], idx / dist grown to the total. Returns the total.
static int64_t thresholdLists(DeviceSession& s, const ismhip_codebook* codewords, int metric, uint32_t n, const float* desc, float threshold) {
    s.act_off.reserve(((size_t)n + 1) * 4);
    int64_t total = 0;
    const int64_t cap = (int64_t)(std::min(s.idx.bytes, s.dist.bytes) / 4);
    s.check(ismhip_knn_threshold(s.ctx, codewords, metric, (int)n, desc, threshold, cap, s.act_off.as<uint32_t>(), s.idx.as<int32_t>(), s.dist.as<float>(), &total),
            "ismhip_knn_threshold");
    if (total > cap) {                                           // the lists did not fit: grow and search again
        s.idx.reserve((size_t)total * 4); s.dist.reserve((size_t)total * 4);
        s.check(ismhip_knn_threshold(s.ctx, codewords, metric, (int)n, desc, threshold, total, s.act_off.as<uint32_t>(), s.idx.as<int32_t>(),
                                     s.dist.as<float>(), &total), "ismhip_knn_threshold");
    }
    return total;
}

// search structure over n_cw codewords only (one dummy vote per word): what the Threshold branch of Codebook::activate searches
static TempCodebook searchOnlyCodebook(DeviceSession& s, uint32_t n_cw, int D, const float* words) {
    std::vector<uint32_t> one((size_t)n_cw + 1), zc(n_cw, 0u);
    std::iota(one.begin(), one.end(), 0u);
    std::vector<float> zxyz((size_t)n_cw * 3, 0.f), sig1(1, 1.f);
    ismhip_codebook* cwb = nullptr;
    s.check(ismhip_codebook_create(s.ctx, (int)n_cw, D, words, nullptr, one.data(), zxyz.data(), nullptr, nullptr, zc.data(), zc.data(),
                                   nullptr, nullptr, 1, sig1.data(), &cwb), "ismhip_codebook_create");
    return TempCodebook(cwb, [&s](ismhip_codebook* cb) { ismhip_codebook_destroy(s.ctx, cb); });
}

// FLANN functors on the host, used by the training statistics only (utils/distance.cpp:33-52)
// Utils::getRotQuaternion + matrix2Quat (utils.cpp:136-151, 342-380): rows of the matrix are the frame axes; out = (w, x, y, z)
static void hostRotQuaternion(const float* l, float* out) {
    const float m[3][3] = {{l[0], l[1], l[2]}, {l[3], l[4], l[5]}, {l[6], l[7], l[8]}};
    float q[4] = {0.f, 0.f, 0.f, 1.f};
    const float trace = m[0][0] + m[1][1] + m[2][2];
    float root;
    if (trace > 0.0f) {
        root = sqrtf(trace + 1.0f); q[3] = 0.5f * root; root = 0.5f / root;
        q[0] = (m[2][1] - m[1][2]) * root; q[1] = (m[0][2] - m[2][0]) * root; q[2] = (m[1][0] - m[0][1]) * root;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        root = sqrtf((float)((double)(m[i][i] - m[j][j] - m[k][k]) + 1.0)); q[i] = 0.5f * root; root = 0.5f / root;
        q[3] = (m[k][j] - m[j][k]) * root; q[j] = (m[j][i] + m[i][j]) * root; q[k] = (m[k][i] + m[i][k]) * root;
    }
    out[0] = q[3]; out[1] = q[0]; out[2] = q[1]; out[3] = q[2];
}
static float hostDistance(int metric, const float* a, const float* b, int n) {
    float result = 0.f;
    if (metric == ISMHIP_METRIC_CHI2) {
        for (int i = 0; i < n; ++i) { const float sum = a[i] + b[i]; if (sum > 0) { const float diff = a[i] - b[i]; result += diff * diff / sum; } }
        return result;
    }
    int i = 0;
    for (; i + 3 < n; i += 4) {
        const float d0 = a[i] - b[i], d1 = a[i + 1] - b[i + 1], d2 = a[i + 2] - b[i + 2], d3 = a[i + 3] - b[i + 3];
        result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    for (; i < n; ++i) { const float d0 = a[i] - b[i]; result += d0 * d0; }
    return result;
}

void Codebook::activate(DeviceSession& s, const DeviceFeatures& f, const std::vector<unsigned>& feat_class, const std::vector<unsigned>& feat_instance,
                        const std::vector<unsigned>& feat_model, const std::vector<std::array<float, 3>>& feat_center,
                        const std::vector<std::array<float, 3>>& feat_bbox_size, int metric, int n_classes, const Clustering& clustering,
                        const std::vector<std::array<float, 4>>* feat_bbox_quat) {
    // codebook.cpp:64-368 with KNN / KNNRule activation; codewords = cluster centres (implicit_shape_model.cpp:445-475), or one per
    // training feature for Clustering "None" (clustering_none.cpp:25-35)
    const uint32_t n = f.n;
    const int D = f.dim;
    if (n == 0) throw RuntimeException("no training features");
    const ActivationStrategy* knn = m_activationStrategy.get();
    const auto* thr = dynamic_cast<const ActivationStrategyThreshold*>(knn);
    const bool is_knn = m_activationStrategy->getType() == "KNN";
    const int k = is_knn ? knn->getK() : 1;                      // KNNRule trains with plain 1-NN (activation_strategy_knn_rule.h:70-74)
    if (k > ISMHIP_KNN_LARGE_K_MAX) throw RuntimeException("KNN activation with K > 1024 (ISMHIP_KNN_LARGE_K_MAX) is not built");
    // the whole of Codebook::activate runs on the device (ismhip_train_activate): self-kNN, class sigma^2, K = 1 clean-up,
    // vote CSR, computeWeights and the statistical class weights. Features must be class-major, as train() collects them.
    const bool clustered = clustering.hasCenters();
    const uint32_t n_cw = clustered ? (uint32_t)clustering.getNumCenters() : n;
    std::vector<uint32_t> cluster_size(n_cw, 1u);                // Codeword::m_numFeatures = clusters[i].size() (:453-473)
    if (clustered) { std::fill(cluster_size.begin(), cluster_size.end(), 0u); for (int ci : clustering.getClusterIndices()) if (ci >= 0 && (uint32_t)ci < n_cw) cluster_size[ci]++; }
    std::vector<float> words((size_t)n_cw * D), centers((size_t)n * 3), lrf, kx, ky, kz;
    if (hipMemcpy(words.data(), clustered ? clustering.getClusterCentersDevice() : f.desc.as<float>(), words.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        throw RuntimeException("hipMemcpy (codewords) failed");
    s.d2h(lrf, f.lrf, (size_t)n * 9); s.d2h(kx, f.kx, n); s.d2h(ky, f.ky, n); s.d2h(kz, f.kz, n);
    for (uint32_t i = 0; i < n; ++i) for (int d = 0; d < 3; ++d) centers[(size_t)i * 3 + d] = feat_center[i][d];
    const bool clean_up = is_knn && k == 1;                     // codebook.cpp:201-224
    int32_t n_words = 0;
    size_t n_act = (size_t)n * k;
    if (thr) {                                                   // Threshold (codebook.cpp:139-142): every codeword below the threshold
        const TempCodebook cwb = searchOnlyCodebook(s, n_cw, D, words.data());
        n_act = (size_t)thresholdLists(s, cwb.get(), metric, n, f.desc.as<float>(), thr->getThreshold());
    }
    std::vector<uint32_t> word_src(n_cw), vote_off((size_t)n_cw + 1), vote_feature(std::max<size_t>(n_act, 1));
    std::vector<float> vote_xyz(std::max<size_t>(n_act, 1) * 3), vote_weight(std::max<size_t>(n_act, 1)), vote_cw(std::max<size_t>(n_act, 1)),
                       sigma((size_t)std::max(1, n_classes));
    if (thr) {
        s.check(ismhip_train_activate_lists(s.ctx, metric, (int)n, D, f.desc.as<float>(), f.lrf.as<float>(), f.kx.as<float>(), f.ky.as<float>(), f.kz.as<float>(),
                                            feat_class.data(), feat_model.data(), centers.data(), (int)n_cw, clustered ? clustering.getClusterCentersDevice() : nullptr,
                                            s.act_off.as<uint32_t>(), s.idx.as<int32_t>(), (int64_t)n_act, std::max(1, n_classes), &n_words, word_src.data(),
                                            vote_off.data(), vote_feature.data(), vote_xyz.data(), vote_weight.data(), vote_cw.data(), sigma.data()),
                "ismhip_train_activate_lists");
    } else {
        s.check(ismhip_train_activate(s.ctx, metric, (int)n, D, f.desc.as<float>(), f.lrf.as<float>(), f.kx.as<float>(), f.ky.as<float>(), f.kz.as<float>(),
                                      feat_class.data(), feat_model.data(), centers.data(), (int)n_cw, clustered ? clustering.getClusterCentersDevice() : nullptr,
                                      k, clean_up ? 1 : 0, std::max(1, n_classes), &n_words, word_src.data(),
                                      vote_off.data(), vote_feature.data(), vote_xyz.data(), vote_weight.data(), vote_cw.data(), sigma.data()), "ismhip_train_activate");
    }
    std::vector<uint32_t> kept(word_src.begin(), word_src.begin() + n_words);
    std::vector<uint32_t> sel(kept.size());
    std::iota(sel.begin(), sel.end(), 0u);
    if (m_use_random_codebook && m_random_codebook_factor < 1.0f) {   // codebook.cpp:821-829, seeded instead of std::random_device
        std::mt19937 rng(0x5EED);
        std::uniform_int_distribution<uint32_t> distr(0, (uint32_t)kept.size());
        std::vector<uint32_t> sub;
        for (uint32_t e : sel) if (!(distr(rng) > m_random_codebook_factor * kept.size())) sub.push_back(e);
        sel.swap(sub);
    }
    CodebookData out; out.dim = D; out.class_sigma = sigma; out.vote_offsets.assign(1, 0u);
    for (uint32_t e : sel) {
        const uint32_t w = kept[e];
        out.words.insert(out.words.end(), words.begin() + (size_t)w * D, words.begin() + (size_t)(w + 1) * D);
        out.word_weight.push_back(1.0f);
        // Codeword(centre, clusters[i].size(), 1.0f, keypoint and class of FEATURE i) (implicit_shape_model.cpp:466-475): with a
        // clustered codebook that is the i-th feature, not a member of cluster i -- kept as the reference has it
        out.word_class.push_back(feat_class[w]);
        out.word_id.push_back((int32_t)w); out.word_num_features.push_back((int32_t)cluster_size[w]);
        out.word_keypoint.push_back(kx[w]); out.word_keypoint.push_back(ky[w]); out.word_keypoint.push_back(kz[w]);
        for (uint32_t v = vote_off[e]; v < vote_off[e + 1]; ++v) {
            const uint32_t fi = vote_feature[v];
            out.vote_xyz.push_back(vote_xyz[(size_t)v * 3]); out.vote_xyz.push_back(vote_xyz[(size_t)v * 3 + 1]); out.vote_xyz.push_back(vote_xyz[(size_t)v * 3 + 2]);
            out.vote_class.push_back(feat_class[fi]); out.vote_instance.push_back(feat_instance[fi]);
            out.vote_weight.push_back(vote_weight[v]); out.vote_class_weight.push_back(vote_cw[v]);
            // addCodeword (codeword_distribution.cpp:63-70): the box in the keypoint's frame, rotQuat = box.rotQuat * conj(q(LRF)); AABB boxes carry (1,0,0,0)
            float q[4]; hostRotQuaternion(&lrf[(size_t)fi * 9], q);
            float bq[4] = {q[0], -q[1], -q[2], -q[3]};
            if (feat_bbox_quat) {                             // the quaternion product a * conj(q), a the box's (MVBB)
                const std::array<float, 4>& a = (*feat_bbox_quat)[fi];
                const float b[4] = {bq[0], bq[1], bq[2], bq[3]};
                bq[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
                bq[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
                bq[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
                bq[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
            }
            out.vote_bbox_quat.insert(out.vote_bbox_quat.end(), bq, bq + 4);
            for (int d = 0; d < 3; ++d) out.vote_bbox_size.push_back(feat_bbox_size[fi][d]);
        }
        out.vote_offsets.push_back((uint32_t)out.vote_class.size());
    }
    LOG_INFO("Size of distribution at the end of training: " << sel.size());
    setData(out);
}

void Codebook::castVotes(DeviceSession& s, const DeviceFeatures& f, int metric, Voting& voting) const {   // codebook.cpp:403-555
    s.n_slots = 0; s.slot_off.assign(s.n_obj + 1, 0);
    if (isEmpty()) return;
    // Voting::vote keeps the keypoint pair of every vote (voting.cpp:58-77); only the RANSAC vote filter reads it
    const bool want_kp = voting.m_vote_filtering_with_ransac;
    if (want_kp && m_data.word_keypoint.size() != (size_t)m_data.numWords() * 3)
        throw RuntimeException("RansacVoteFiltering needs the codewords' training keypoints, which this codebook does not hold");
    upload(s);
    m_activationStrategy->setIsDetection();
    const ActivationStrategy* knn = m_activationStrategy.get();
    if (knn->getK() > ISMHIP_KNN_LARGE_K_MAX) throw RuntimeException("KNN activation with K > 1024 (ISMHIP_KNN_LARGE_K_MAX) is not built");
    const uint32_t n = f.n;
    if (n == 0) return;
    const size_t kmax = (size_t)std::max(knn->getK(), 1);          // activations per feature of the K-nearest strategies
    const size_t kres = std::max<size_t>(kmax, 4);                // (at least the 4 per feature this buffer always had: Threshold grows from it)
    s.idx.reserve((size_t)n * kres * 4); s.dist.reserve((size_t)n * kres * 4);
    const float* qdesc = nullptr;
    DevBuf partial;
    if (!m_partial_cols.empty()) {                              // reduce every feature the way the codewords were reduced (codebook.cpp:416-475)
        if (f.dim != ISMHIP_SHOT_DIM) throw RuntimeException("UsePartialShot needs SHOT-352 features");
        partial.reserve((size_t)n * m_partial_cols.size() * 4);
        s.check(ismhip_gather_columns(s.ctx, (int)n, f.dim, f.desc.as<float>(), (int)m_partial_cols.size(), m_partial_cols.data(), partial.as<float>()), "ismhip_gather_columns");
        qdesc = partial.as<float>();
    }
    const uint32_t flags = (m_useClassWeight ? ISMHIP_W_CLASS : 0u) | (m_useVoteWeight ? ISMHIP_W_VOTE : 0u) |
                           (m_useMatchingWeight ? ISMHIP_W_MATCHING : 0u) | (m_useCodewordWeight ? ISMHIP_W_CODEWORD : 0u);
    const auto* thr = dynamic_cast<const ActivationStrategyThreshold*>(knn);
    const int maxv = ismhip_codebook_max_votes_per_word(m_dev);
    int64_t na = 0;                                               // activations of the batch
    int k = 0;                                                    // per feature (K-nearest strategies)
    if (thr) {
        // list path (codebook.cpp:505-508): every activated codeword casts all its votes; slot of (activation a, vote v) = a*maxv + v
        na = thresholdLists(s, m_dev, metric, n, qdesc ? qdesc : f.desc.as<float>(), thr->getThreshold());
    } else {
        // refuse what would not fit rather than truncate: ismhip_cast_votes counts activations in an int, vote slots are addressed with
        // 32 bits (slot_off, ismhip_find_maxima)
        if ((uint64_t)n * kmax > 0x7fffffffull)
            throw RuntimeException("castVotes: features x K reaches 2^31 activations, not built");
        if ((uint64_t)n * kmax * (uint64_t)std::max(maxv, 1) >= (1ull << 32))
            throw RuntimeException("castVotes: features x K x votes per codeword reaches 2^32 vote slots, not built");
        k = knn->activateKNN(s, m_dev, f, metric, s.idx.as<int32_t>(), s.dist.as<float>(), qdesc);
        if (qdesc) s.check(ismhip_sync(s.ctx), "ismhip_sync");     // the partial descriptors are released when this function returns
        na = (int64_t)n * k;
    }
    const size_t ns = (size_t)na * maxv;
    s.v_pos.reserve(ns * 12); s.v_w.reserve(ns * 4); s.v_cls.reserve(ns * 4); s.v_inst.reserve(ns * 4); s.v_cw.reserve(ns * 4); s.v_bs.reserve(ns * 12); s.v_bq.reserve(ns * 16);
    if (want_kp) { s.v_kp.reserve(ns * 12); s.v_kpt.reserve(ns * 12); }
    const float *lrf = f.lrf.as<float>(), *kx = f.kx.as<float>(), *ky = f.ky.as<float>(), *kz = f.kz.as<float>();
    const uint32_t* act_off = s.act_off.as<uint32_t>();
    const int32_t* idx = s.idx.as<int32_t>();
    if (thr) {
        s.check(ismhip_cast_votes_csr(s.ctx, m_dev, flags, (int)n, lrf, kx, ky, kz, act_off, na, idx, s.dist.as<float>(), s.v_pos.as<float>(), s.v_w.as<float>(),
                                      s.v_cls.as<int32_t>(), s.v_inst.as<int32_t>(), s.v_cw.as<int32_t>(), s.v_bq.as<float>(), s.v_bs.as<float>()), "ismhip_cast_votes_csr");
        if (want_kp) s.check(ismhip_vote_keypoints_csr(s.ctx, m_dev, (int)n, kx, ky, kz, act_off, na, idx, s.v_kp.as<float>(), s.v_kpt.as<float>()), "ismhip_vote_keypoints_csr");
    } else {
        s.check(ismhip_cast_votes(s.ctx, m_dev, flags, (int)n, lrf, kx, ky, kz, k, idx, s.dist.as<float>(), s.v_pos.as<float>(), s.v_w.as<float>(),
                                  s.v_cls.as<int32_t>(), s.v_inst.as<int32_t>(), s.v_cw.as<int32_t>(), s.v_bq.as<float>(), s.v_bs.as<float>()), "ismhip_cast_votes");
        if (want_kp) s.check(ismhip_vote_keypoints(s.ctx, m_dev, (int)n, kx, ky, kz, k, idx, s.v_kp.as<float>(), s.v_kpt.as<float>()), "ismhip_vote_keypoints");
    }
    // an object's first slot: its first activation (list path: from the activation ranges; K-nearest: k per feature) times maxv
    std::vector<uint32_t> first_act;
    if (thr) s.d2h(first_act, s.act_off, (size_t)n + 1);
    s.n_slots = ns;
    for (int o = 0; o <= s.n_obj; ++o) s.slot_off[o] = (thr ? first_act[f.off[o]] : f.off[o] * (uint32_t)k) * (uint32_t)maxv;
    s.n_classes = (int)m_data.class_sigma.size();
}

std::string CodebookData::validate() const {
    const size_t nw = (size_t)numWords(), nv = vote_offsets.empty() ? 0 : vote_offsets.back();
    if (dim <= 0 || words.size() % (size_t)dim) return "descriptor length does not divide the word array";
    if (vote_offsets.size() != nw + 1 || vote_offsets[0] != 0) return "vote offsets do not match the number of codewords";
    for (size_t i = 0; i < nw; ++i) if (vote_offsets[i + 1] < vote_offsets[i]) return "vote offsets not monotone";
    if (vote_xyz.size() != nv * 3 || vote_class.size() != nv || vote_instance.size() != nv) return "vote arrays do not match the vote offsets";
    if (!vote_weight.empty() && vote_weight.size() != nv) return "vote weights do not match the vote offsets";
    if (!vote_class_weight.empty() && vote_class_weight.size() != nv) return "class weights do not match the vote offsets";
    if (!vote_bbox_quat.empty() && vote_bbox_quat.size() != nv * 4) return "bounding-box quaternions do not match the vote offsets";
    if (!vote_bbox_size.empty() && vote_bbox_size.size() != nv * 3) return "bounding-box sizes do not match the vote offsets";
    if (!word_weight.empty() && word_weight.size() != nw) return "word weights do not match the number of codewords";
    if (!word_class.empty() && word_class.size() != nw) return "word classes do not match the number of codewords";
    if (class_sigma.empty()) return "no class sigmas";
    for (uint32_t c : vote_class) if (c >= class_sigma.size()) return "vote class id beyond the class sigmas";
    return "";
}

// Codebook::iSaveData (codebook.cpp:739-761) -> CodewordDistribution::iSaveData (codeword_distribution.cpp:349-391) ->
// Codeword::iSaveData (codeword.cpp:71-83), field by field
void Codebook::save(BoostBinaryOArchive& oa) const {
    const CodebookData& d = m_data;
    const int nw = d.numWords();
    oa << nw;                                                                     // distribution_size
    for (int w = 0; w < nw; ++w) {
        // Codeword: m_id, m_numFeatures, m_weight, m_data, m_class_id, keypoint xyz
        oa << (d.word_id.empty() ? w : (int)d.word_id[w]) << (d.word_num_features.empty() ? 1 : (int)d.word_num_features[w])
           << (d.word_weight.empty() ? 1.0f : d.word_weight[w]);
        oa << std::vector<float>(d.words.begin() + (size_t)w * d.dim, d.words.begin() + (size_t)(w + 1) * d.dim);
        const uint32_t v0 = d.vote_offsets[w], v1 = d.vote_offsets[w + 1];
        oa << (int)(d.word_class.empty() ? (v1 > v0 ? d.vote_class[v0] : 0u) : d.word_class[w]);
        for (int k = 0; k < 3; ++k) oa << (d.word_keypoint.empty() ? 0.0f : d.word_keypoint[(size_t)w * 3 + k]);
        // distribution: votes, m_weights, m_class_ids, m_instance_ids, m_classWeights (std::map: ascending class), bounding boxes
        oa << (int)(v1 - v0);
        for (uint32_t v = v0; v < v1; ++v) oa << d.vote_xyz[(size_t)v * 3] << d.vote_xyz[(size_t)v * 3 + 1] << d.vote_xyz[(size_t)v * 3 + 2];
        oa << (d.vote_weight.empty() ? std::vector<float>(v1 - v0, 1.0f) : std::vector<float>(d.vote_weight.begin() + v0, d.vote_weight.begin() + v1));
        oa << std::vector<unsigned>(d.vote_class.begin() + v0, d.vote_class.begin() + v1);
        oa << std::vector<unsigned>(d.vote_instance.begin() + v0, d.vote_instance.begin() + v1);
        std::map<unsigned, float> cw;
        for (uint32_t v = v0; v < v1; ++v) cw[d.vote_class[v]] = d.vote_class_weight.empty() ? 1.0f : d.vote_class_weight[v];
        oa << (int)cw.size();
        for (auto& kv : cw) oa << (int)kv.first << kv.second;
        oa << (int)(v1 - v0);
        for (uint32_t v = v0; v < v1; ++v) {
            for (int k = 0; k < 4; ++k) oa << (d.vote_bbox_quat.empty() ? (k == 0 ? 1.0f : 0.0f) : d.vote_bbox_quat[(size_t)v * 4 + k]);
            for (int k = 0; k < 3; ++k) oa << (d.vote_bbox_size.empty() ? 0.0f : d.vote_bbox_size[(size_t)v * 3 + k]);
        }
    }
    // m_classSigmas (std::map<unsigned, float>): only classes that were trained have an entry
    int n_sig = 0;
    for (float sg : d.class_sigma) if (sg == sg) ++n_sig;      // NaN marks a class id that was never trained: no map entry
    oa << n_sig;
    for (size_t c = 0; c < d.class_sigma.size(); ++c) if (d.class_sigma[c] == d.class_sigma[c]) oa << (int)c << d.class_sigma[c];
    // m_activationStrategy->saveData: nothing (json_object.cpp:256-259)
}

bool Codebook::load(BoostBinaryIArchive& ia) {
    CodebookData d;
    int nw = 0; ia >> nw;
    if (!ia.ok() || nw < 0 || !ia.plausible((uint64_t)nw, 60)) return false;
    LOG_INFO("Loading codebook with size: " << nw);
    std::mt19937 rng(0x5EED);                                  // UseRandomCodebook (codebook.cpp:821-829), seeded instead of std::random_device
    std::uniform_int_distribution<int> pick(0, nw);
    std::map<unsigned, float> sig_map;
    for (int w = 0; w < nw && ia.ok(); ++w) {
        int id = 0, nf = 0, cls = 0; float weight = 0.f, kp[3] = {0, 0, 0};
        std::vector<float> data, weights; std::vector<unsigned> class_ids, instance_ids;
        ia >> id >> nf >> weight >> data >> cls >> kp[0] >> kp[1] >> kp[2];
        int votes = 0; ia >> votes;
        if (!ia.ok() || votes < 0 || !ia.plausible((uint64_t)votes, 12)) return false;
        std::vector<float> vxyz((size_t)votes * 3);
        for (float& x : vxyz) ia >> x;
        ia >> weights >> class_ids >> instance_ids;
        int ncw = 0; ia >> ncw;
        if (!ia.ok() || ncw < 0 || !ia.plausible((uint64_t)ncw, 8)) return false;
        std::map<unsigned, float> cw;
        for (int i = 0; i < ncw; ++i) { int c = 0; float x = 0.f; ia >> c >> x; cw[(unsigned)c] = x; }
        int nbb = 0; ia >> nbb;
        if (!ia.ok() || nbb < 0 || !ia.plausible((uint64_t)nbb, 28)) return false;
        std::vector<float> bq((size_t)nbb * 4), bs((size_t)nbb * 3);
        for (int i = 0; i < nbb; ++i) { for (int k = 0; k < 4; ++k) ia >> bq[(size_t)i * 4 + k]; for (int k = 0; k < 3; ++k) ia >> bs[(size_t)i * 3 + k]; }
        if (!ia.ok()) return false;
        if ((int)weights.size() != votes || (int)class_ids.size() != votes || (int)instance_ids.size() != votes || nbb != votes) { ia.fail("codeword distribution arrays of unequal length"); return false; }
        if (d.dim == 0) d.dim = (int)data.size();
        if ((int)data.size() != d.dim || d.dim == 0) { ia.fail("codewords of different descriptor length"); return false; }
        if (m_use_random_codebook && pick(rng) > m_random_codebook_factor * nw) continue;      // skip features while loading (:821-829)
        d.words.insert(d.words.end(), data.begin(), data.end());
        d.word_id.push_back(id); d.word_num_features.push_back(nf); d.word_weight.push_back(weight); d.word_class.push_back((uint32_t)cls);
        d.word_keypoint.insert(d.word_keypoint.end(), kp, kp + 3);
        d.vote_xyz.insert(d.vote_xyz.end(), vxyz.begin(), vxyz.end());
        d.vote_weight.insert(d.vote_weight.end(), weights.begin(), weights.end());
        d.vote_class.insert(d.vote_class.end(), class_ids.begin(), class_ids.end());
        d.vote_instance.insert(d.vote_instance.end(), instance_ids.begin(), instance_ids.end());
        for (unsigned c : class_ids) { auto it = cw.find(c); d.vote_class_weight.push_back(it == cw.end() ? 1.0f : it->second); }   // castVotes: 1 + warning when missing (:97-104)
        d.vote_bbox_quat.insert(d.vote_bbox_quat.end(), bq.begin(), bq.end()); d.vote_bbox_size.insert(d.vote_bbox_size.end(), bs.begin(), bs.end());
        d.vote_offsets.push_back((uint32_t)d.vote_class.size());
    }
    int n_sig = 0; ia >> n_sig;
    if (!ia.ok() || n_sig < 0 || !ia.plausible((uint64_t)n_sig, 8)) return false;
    unsigned max_class = 0;
    for (int i = 0; i < n_sig; ++i) { int c = 0; float sg = 0.f; ia >> c >> sg; if (c < 0 || c > (1 << 20)) { ia.fail("class id out of range"); return false; } sig_map[(unsigned)c] = sg; max_class = std::max(max_class, (unsigned)c); }
    for (unsigned c : d.vote_class) max_class = std::max(max_class, c);
    if (max_class > (1u << 20)) { ia.fail("class id out of range"); return false; }
    d.class_sigma.assign((size_t)max_class + 1, 1.0f);          // castVotes uses sigma 1 (+ warning) for a class without an entry (:108-117)
    for (auto& kv : sig_map) d.class_sigma[kv.first] = kv.second;
    if (!ia.ok()) return false;
    const std::string why = d.validate();
    if (!why.empty()) { ia.fail("inconsistent codebook: " + why); return false; }
    if (m_use_random_codebook) LOG_INFO("Reduced codebook size: " << d.numWords());
    setData(d);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// Global descriptors (features/features_short_shot_global.cpp, features_shot_global.cpp, features_vfh.cpp, features_gasd.cpp) on regions of the batch's search surface
// ---------------------------------------------------------------------------------------------------------------
struct GlobalRegions {
    int n = 0, dim = 0;
    DevBuf obj, cen, rad;                          // the regions
    DevBuf n_sel, centroid, radius, lrf, desc;     // the outputs
    // rows of region r: row_off[r] .. row_off[r + 1] of desc and lrf. One each, set here; only CVFH's describe() rewrites it
    std::vector<uint32_t> row_off;
    size_t rows() const { return row_off.empty() ? 0 : row_off.back(); }
    // uploads the regions and reserves the outputs for rows of `dim` floats
    void set(const std::vector<int32_t>& o, const std::vector<float>& c, const std::vector<float>& r, int D) {
        n = (int)o.size(); dim = D;
        row_off.resize((size_t)n + 1); std::iota(row_off.begin(), row_off.end(), 0u);
        DeviceSession::h2d(obj, o); DeviceSession::h2d(cen, c); DeviceSession::h2d(rad, r);
        const size_t m = std::max<size_t>((size_t)n, 1);
        n_sel.reserve(m * 4); centroid.reserve(m * 12); radius.reserve(m * 4); lrf.reserve(m * 36); desc.reserve(m * (size_t)D * 4);
    }
};
GlobalFeaturesShortShot::GlobalFeaturesShortShot() {          // features_short_shot_global.cpp:21-30
    addParameter(m_min_radius, "ShortShotMinRadius", 0.1);
    addParameter(m_feature_dims, "ShortShotDims", 32);
    addParameter(m_log_radius, "ShortShotLogRadius", false);
    addParameter(m_r_bins, "ShortShotRBins", 1);
    addParameter(m_e_bins, "ShortShotEBins", 1);
    addParameter(m_a_bins, "ShortShotABins", 8);
    addParameter(m_bin_type, "ShortShotBinType", std::string("auto"));
}
void GlobalFeaturesShortShot::iPostInitConfig() {             // configureSphericalGrid (:168-249); 64 is 4 x 2 x 8 here, unlike the local descriptor
    static const int sizes[9][4] = {{8, 1, 1, 8}, {16, 2, 2, 4}, {24, 2, 2, 6}, {32, 2, 2, 8}, {64, 4, 2, 8}, {96, 3, 4, 8}, {128, 4, 4, 8}, {192, 6, 4, 8}, {256, 8, 4, 8}};
    if (m_bin_type == "manual") {
        if (m_r_bins < 1 || m_e_bins < 1 || m_a_bins < 1 || (long long)m_r_bins * m_e_bins * m_a_bins > ISMHIP_SHORT_SHOT_MAX_DIM)
            throw RuntimeException("SHORT_SHOT_GLOBAL: " + std::to_string(m_r_bins) + " x " + std::to_string(m_e_bins) + " x " + std::to_string(m_a_bins) +
                                   " bins are not built (built: 1 .. " + std::to_string(ISMHIP_SHORT_SHOT_MAX_DIM) + " bins)");
        m_feature_dims = m_r_bins * m_e_bins * m_a_bins;
        return;
    }
    const int* hit = nullptr;
    if (m_bin_type == "auto") for (auto& row : sizes) if (row[0] == m_feature_dims) hit = row;
    if (!hit) {
        if (m_bin_type == "auto") LOG_ERROR("Unsupported Short SHOT dimensions for automatic bin configuration: " << m_feature_dims << "! Setting to 32 dimensions with default bins.");
        else LOG_ERROR("Unsupported Short SHOT bins configuration type: " << m_bin_type << "! Setting to 32 dimensions with default bins.");
        hit = sizes[3];
    }
    m_feature_dims = hit[0]; m_r_bins = hit[1]; m_e_bins = hit[2]; m_a_bins = hit[3];
    if (m_log_radius && !(m_min_radius > 0)) throw RuntimeException("SHORT_SHOT_GLOBAL: ShortShotLogRadius needs ShortShotMinRadius > 0");
}
void GlobalFeaturesShortShot::describe(DeviceSession& s, GlobalRegions& r) const {
    s.check(ismhip_global_short_shot(s.ctx, s.cloud, r.n, r.obj.as<int32_t>(), r.cen.as<float>(), r.rad.as<float>(), m_min_radius, m_log_radius ? 1 : 0,
                                     m_r_bins, m_e_bins, m_a_bins, r.n_sel.as<uint32_t>(), r.centroid.as<float>(), r.radius.as<float>(), r.lrf.as<float>(),
                                     r.desc.as<float>(), nullptr), "ismhip_global_short_shot");
}
void GlobalFeaturesShot::describe(DeviceSession& s, GlobalRegions& r) const {
    s.check(ismhip_global_shot352(s.ctx, s.cloud, r.n, r.obj.as<int32_t>(), r.cen.as<float>(), r.rad.as<float>(), r.n_sel.as<uint32_t>(), r.centroid.as<float>(),
                                  r.radius.as<float>(), r.lrf.as<float>(), r.desc.as<float>()), "ismhip_global_shot352");
}
void GlobalFeaturesVFH::describe(DeviceSession& s, GlobalRegions& r) const {
    const float viewpoint[3] = {0.f, 0.f, 0.f};                                       // PCL's default, which features_vfh.cpp leaves
    DevBuf ncen; ncen.reserve(std::max<size_t>((size_t)r.n, 1) * 12);
    s.check(ismhip_global_vfh(s.ctx, s.cloud, r.n, r.obj.as<int32_t>(), r.cen.as<float>(), r.rad.as<float>(), viewpoint, 0, r.n_sel.as<uint32_t>(),
                              r.centroid.as<float>(), r.radius.as<float>(), ncen.as<float>(), r.desc.as<float>(), nullptr), "ismhip_global_vfh");
    DeviceSession::h2d(r.lrf, std::vector<float>((size_t)r.n * 9, 0.f));             // VFH has no frame: the stored rf of a row is zeros
    s.sync();                                                                         // ncen is released on return
}
GlobalFeaturesGASD::GlobalFeaturesGASD() { addParameter(m_use_color, "GasdWithColor", true); }   // features_gasd.cpp:16-19
void GlobalFeaturesGASD::checkInput(const PointCloud& cloud) const {
    if (m_use_color && !cloud.empty() && cloud.rgba.size() != cloud.size()) throw RuntimeException("GASD needs coloured point clouds");
}
void GlobalFeaturesGASD::describe(DeviceSession& s, GlobalRegions& r) const {
    if (m_use_color && !s.has_color) throw RuntimeException("GASD needs coloured point clouds");
    const float view_direction[3] = {0.f, 0.f, 1.f};                                  // PCL's default, which features_gasd.cpp leaves
    DevBuf frame, max_coord;
    frame.reserve(std::max<size_t>((size_t)r.n, 1) * 36); max_coord.reserve(std::max<size_t>((size_t)r.n, 1) * 4);
    s.check(ismhip_global_gasd(s.ctx, s.cloud, r.n, r.obj.as<int32_t>(), r.cen.as<float>(), r.rad.as<float>(), view_direction, m_use_color ? 1 : 0,
                               r.n_sel.as<uint32_t>(), r.centroid.as<float>(), r.radius.as<float>(), frame.as<float>(), max_coord.as<float>(),
                               r.desc.as<float>(), nullptr), "ismhip_global_gasd");
    // the reference leaves ISMFeature::referenceFrame untouched for this type (its constructor does not initialise it): zeros, as for VFH
    DeviceSession::h2d(r.lrf, std::vector<float>((size_t)r.n * 9, 0.f));
    s.sync();                                                                         // frame and max_coord are released on return
}
GlobalFeaturesCVFH::GlobalFeaturesCVFH() {                    // PCL's defaults for a leaf size of 0.005 (cvfh.h); the reference sets none of them
    addParameter(m_cluster_tolerance, "CvfhClusterTolerance", 0.015);
    addParameter(m_normal_radius, "CvfhNormalRadius", 0.015);
    addParameter(m_min_points, "CvfhMinPoints", 50);
}
void GlobalFeaturesCVFH::describe(DeviceSession& s, GlobalRegions& r) const {
    if (!(m_cluster_tolerance > 0) || m_min_points < 1) throw RuntimeException("CVFH: CvfhClusterTolerance must be positive and CvfhMinPoints at least 1");
    const float viewpoint[3] = {0.f, 0.f, 0.f};                                       // PCL's default, which features_cvfh.cpp leaves
    const double angle = 10.0 / 180.0 * M_PI;                                         // features_cvfh.cpp
    const size_t n = (size_t)r.n, m = std::max<size_t>(n, 1);
    DevBuf ncl, rcen, rnrm, rsize, rows;
    std::vector<uint32_t> counts;
    int cap = 4;                                                                      // rows per region the buffers hold; a region with more: once more
    for (;;) {
        ncl.reserve(m * 4); rcen.reserve(m * cap * 12); rnrm.reserve(m * cap * 12); rsize.reserve(m * cap * 4);
        rows.reserve(m * cap * (size_t)ISMHIP_VFH_DIM * 4);
        s.check(ismhip_global_cvfh(s.ctx, s.cloud, r.n, r.obj.as<int32_t>(), r.cen.as<float>(), r.rad.as<float>(), viewpoint, (float)m_cluster_tolerance,
                                   (float)m_normal_radius, m_min_points, angle, cap, r.n_sel.as<uint32_t>(), r.centroid.as<float>(), r.radius.as<float>(),
                                   ncl.as<uint32_t>(), rcen.as<float>(), rnrm.as<float>(), rsize.as<uint32_t>(), rows.as<float>(), nullptr, nullptr),
                "ismhip_global_cvfh");
        s.d2h(counts, ncl, n);
        uint32_t most = 0;
        for (uint32_t c : counts) most = std::max(most, c);
        if (most <= (uint32_t)cap) break;
        cap = (int)most;
    }
    std::vector<float> all, packed;
    s.d2h(all, rows, n * cap * (size_t)ISMHIP_VFH_DIM);
    r.row_off.assign(1, 0u);
    for (size_t i = 0; i < n; ++i) {
        packed.insert(packed.end(), all.begin() + i * cap * ISMHIP_VFH_DIM, all.begin() + (i * cap + counts[i]) * ISMHIP_VFH_DIM);
        r.row_off.push_back(r.row_off.back() + counts[i]);
    }
    if (packed.empty()) packed.assign(1, 0.f);
    DeviceSession::h2d(r.desc, packed);
    DeviceSession::h2d(r.lrf, std::vector<float>(std::max<size_t>(r.rows(), 1) * 9, 0.f));   // no frame: the stored rf of a row is zeros, as for VFH
    s.sync();
}
GlobalFeatures* GlobalFeatures::createIfBuilt(const Json& object) {
    if (!object.isObject()) return nullptr;
    const Json* t = object.find("Type");
    if (!t || t->type != Json::String) return nullptr;
    GlobalFeatures* g = nullptr;
    if (t->str == GlobalFeaturesShortShot::getTypeStatic()) g = new GlobalFeaturesShortShot();
    else if (t->str == GlobalFeaturesShot::getTypeStatic()) g = new GlobalFeaturesShot();
    else if (t->str == GlobalFeaturesVFH::getTypeStatic()) g = new GlobalFeaturesVFH();
    else if (t->str == GlobalFeaturesGASD::getTypeStatic()) g = new GlobalFeaturesGASD();
    else if (t->str == GlobalFeaturesCVFH::getTypeStatic()) g = new GlobalFeaturesCVFH();
    if (!g) return nullptr;
    try { if (!g->configFromJson(object)) throw RuntimeException("could not create object of type: \"" + t->str + "\""); }
    catch (...) { delete g; throw; }
    return g;
}

// GlobalClassifier::classifyWithKNN (global_classifier.cpp:242-347) with insertGlobalResult / GlobalResultAccu (.h:33-62): per class the
// occurrences and the float score sum, per instance of the class likewise; std::map order, so a tie goes to the lowest id
VotingMaximum::GlobalHypothesis Voting::classifyWithKNN(int k, const unsigned* n_class, const unsigned* n_inst, const float* n_dist, unsigned max_class,
                                                         bool single_object_mode) {
    struct Accu { unsigned n = 0; float score = 0; std::map<unsigned, std::pair<int, float>> inst; };
    std::map<unsigned, Accu> votes;
    for (int i = 0; i < k; ++i) {
        const float score = std::exp(-std::sqrt(n_dist[i]));            // float sqrt, float exp
        Accu& a = votes[n_class[i]];
        a.n++; a.score += score;
        auto& e = a.inst[n_inst[i]];
        e.first++; e.second += score;
    }
    VotingMaximum::GlobalHypothesis g; g.classId = max_class;
    auto best_instance = [&](const Accu& a) {
        int best = 0;
        for (auto& it : a.inst) if (it.second.first > best) { best = it.second.first; g.instanceId = it.first; }
        const auto& e = a.inst.at(g.instanceId);
        g.instanceWeight = e.second / e.first;
    };
    if (single_object_mode) {
        if (votes.empty()) return g;                                    // (the reference would throw from map::at)
        unsigned best = 0;
        for (auto& it : votes) if (it.second.n > best) { best = it.second.n; g.classId = it.first; }
        const Accu& a = votes.at(g.classId);
        g.classWeight = a.score / a.n;
        best_instance(a);
    } else {
        auto it = votes.find(max_class);
        if (it != votes.end()) { g.classWeight = it->second.n > 0 ? it->second.score / it->second.n : 0; best_instance(it->second); }
    }
    return g;
}

// Voting::normalizeWeights (voting.cpp:441-462)
static void normalizeMaxima(std::vector<VotingMaximum>& maxima) {
    float sum = 0, sum_instance = 0, sum_global = 0, sum_instance_global = 0;
    for (const VotingMaximum& m : maxima) { sum += m.weight; sum_instance += m.instanceWeight; sum_global += m.globalHypothesis.classWeight; sum_instance_global += m.globalHypothesis.instanceWeight; }
    for (VotingMaximum& m : maxima) {
        m.weight = sum != 0 ? m.weight / sum : 0;
        m.instanceWeight = sum_instance != 0 ? m.instanceWeight / sum_instance : 0;
        m.globalHypothesis.classWeight = sum_global != 0 ? m.globalHypothesis.classWeight / sum_global : 0;
        m.globalHypothesis.instanceWeight = sum_instance_global != 0 ? m.globalHypothesis.instanceWeight / sum_instance_global : 0;
    }
}
// GlobalClassifier::useHighRankedGlobalHypothesis (global_classifier.cpp:579-601)
static void useHighRankedGlobalHypothesis(std::vector<VotingMaximum>& maxima, float rate_limit) {
    const float top_weight = maxima[0].weight;
    const unsigned global_class = maxima[0].globalHypothesis.classId;
    for (size_t i = 0; i < maxima.size(); ++i) {
        const float cur_weight = maxima[i].weight;
        if (cur_weight >= top_weight * rate_limit && maxima[i].classId == global_class) {
            maxima[0].classId = maxima[0].globalHypothesis.classId; maxima[0].instanceId = maxima[0].globalHypothesis.instanceId;
            break;
        } else if (cur_weight < top_weight * rate_limit) break;
    }
}
static float norm3(float x, float y, float z) { return std::sqrt(x * x + y * y + z * z); }
void Voting::mergeSequence(std::vector<VotingMaximum>& maxima, const MergeParams& p) {
    auto by_weight = [](const VotingMaximum& a, const VotingMaximum& b) { return a.weight > b.weight; };
    std::stable_sort(maxima.begin(), maxima.end(), by_weight);                       // the reference's std::sort leaves the order of equal weights open
    if (maxima.empty()) return;
    if (p.function != 5) normalizeMaxima(maxima);                                    // :278-282
    // mergeGlobalAndLocalHypotheses (global_classifier.cpp:457-577)
    const int fn = p.function;
    auto near = [&](const VotingMaximum& m) {
        const auto& c = m.roiCentroid;
        if (norm3(c[0], c[1], c[2]) == 0) return true;                               // classification, not detection
        return norm3(m.position[0] - c[0], m.position[1] - c[1], m.position[2] - c[2]) < p.radius / 2.0f;
    };
    if (fn == 1) {
        if (maxima[0].globalHypothesis.classWeight > p.min_svm_score) { maxima[0].classId = maxima[0].globalHypothesis.classId; maxima[0].instanceId = maxima[0].globalHypothesis.instanceId; }
    } else if (fn == 2) {
        if (maxima[0].globalHypothesis.classWeight > p.min_svm_score) useHighRankedGlobalHypothesis(maxima, p.rate_limit);
    } else if (fn == 3) {
        useHighRankedGlobalHypothesis(maxima, p.rate_limit);
    } else if (fn == 4) {
        for (VotingMaximum& m : maxima) {
            const bool ok = near(m);
            if (m.classId == m.globalHypothesis.classId && ok) { if (m.globalHypothesis.classWeight == 0) m.weight = 0; else m.weight *= p.weight_factor; }
            if (m.instanceId == m.globalHypothesis.instanceId && ok) { if (m.globalHypothesis.instanceWeight == 0) m.instanceWeight = 0; else m.instanceWeight *= p.weight_factor; }
        }
    } else if (fn == 5) {
        for (VotingMaximum& m : maxima)
            if (near(m)) {
                if (m.classId == m.globalHypothesis.classId) m.weight *= 1 + m.globalHypothesis.classWeight;
                if (m.instanceId == m.globalHypothesis.instanceId) m.instanceWeight *= 1 + m.globalHypothesis.instanceWeight;
            }
    } else if (fn == 6) {
        for (VotingMaximum& m : maxima) {
            if (m.classId == m.globalHypothesis.classId) m.weight *= m.globalHypothesis.classWeight;
            if (m.instanceId == m.globalHypothesis.instanceId) m.instanceWeight *= m.globalHypothesis.instanceWeight;
        }
    } else if (fn == 7) {
        for (VotingMaximum& m : maxima)
            if (m.classId == m.globalHypothesis.classId && near(m)) {
                float w1 = m.weight, w2 = m.globalHypothesis.classWeight;
                m.weight = w1 + w2 - w1 * w2;
                if (m.instanceId == m.globalHypothesis.instanceId) { w1 = m.instanceWeight; w2 = m.globalHypothesis.instanceWeight; m.instanceWeight = w1 + w2 - w1 * w2; }
            }
    } else {
        LOG_ERROR("Invalid merging function specified: " << fn << "! Not merging local and global hypotheses.");
    }
    std::stable_sort(maxima.begin(), maxima.end(), by_weight);                       // :287
    maxima.erase(std::find_if(maxima.begin(), maxima.end(), [](const VotingMaximum& m) { return m.weight == 0; }), maxima.end());
    normalizeMaxima(maxima);                                                         // :298
    float weight_threshold = p.min_threshold;                                        // :304-323
    if (weight_threshold < 0) weight_threshold = -weight_threshold * (maxima.empty() ? 0.0f : maxima.front().weight);
    std::vector<VotingMaximum> kept;
    for (const VotingMaximum& m : maxima) if (m.weight >= weight_threshold) kept.push_back(m);
    maxima.swap(kept);
    if (p.best_k > 0 && (int)maxima.size() >= p.best_k) maxima.erase(maxima.begin() + p.best_k, maxima.end());
}

// Voting::forwardBoxesAndRadii (voting.cpp:496-551)
void Voting::forwardBoxesAndRadii(const std::map<unsigned, std::vector<std::array<float, 3>>>& box_sizes, const std::map<unsigned, std::vector<float>>& object_radii) {
    m_dimensions_map.clear(); m_variance_map.clear();
    for (auto& it : box_sizes) {
        const unsigned classId = it.first;
        float median_box_dim = 0, median_box_dim_squared = 0;
        for (auto& size : it.second) {
            const float mx = std::max(size[0], std::max(size[1], size[2])), mn = std::min(size[0], std::min(size[1], size[2]));
            float med = size[0];                               // "find the other value" (:512-520)
            for (int i = 1; i < 3; ++i) if (med == mx || med == mn) med = size[i];
            median_box_dim += med; median_box_dim_squared += med * med;
        }
        float class_radii = 0, class_radii_squared = 0;
        auto rit = object_radii.find(classId);
        if (rit != object_radii.end()) for (float r : rit->second) { class_radii += r; class_radii_squared += r * r; }
        const float n = (float)it.second.size();
        median_box_dim /= n; median_box_dim_squared /= n; class_radii /= n; class_radii_squared /= n;
        m_dimensions_map[classId] = {class_radii, median_box_dim};
        m_variance_map[classId] = {class_radii_squared - class_radii * class_radii, median_box_dim_squared - median_box_dim * median_box_dim};
    }
}
// MaximaHandler::getSearchDistForClass (maxima_handler.cpp:509-521)
std::vector<float> Voting::searchDistPerClass(float radius, int n_classes) const {
    if (m_radiusType == "Config" || m_radiusType == "Fixed") return {};
    const bool first = m_radiusType == "FirstDim" || m_radiusType == "ObjectRadius", second = m_radiusType == "SecondDim" || m_radiusType == "BoundingBoxMedian";
    if (!first && !second) { LOG_ERROR("Invalid radius type: " << m_radiusType << "! Using config value instead."); return {}; }
    std::vector<float> out((size_t)n_classes, radius);
    for (int c = 0; c < n_classes; ++c) {
        auto it = m_dimensions_map.find((unsigned)c);
        if (it == m_dimensions_map.end()) continue;            // a class that was never trained casts no votes either
        out[c] = (first ? it->second.first : it->second.second) * m_radiusFactor;
    }
    return out;
}
void Voting::save(BoostBinaryOArchive& oa) const {
    oa << (unsigned)m_dimensions_map.size();
    for (auto& it : m_dimensions_map) oa << it.first << it.second.first << it.second.second;
    oa << (unsigned)m_variance_map.size();
    for (auto& it : m_variance_map) oa << it.first << it.second.first << it.second.second;
    // global features (voting.cpp:586-613): per class its training clouds, per cloud its rows -- nine frame floats, the descriptor
    // vector, the radius, the instance id. A model without a built global descriptor writes none.
    oa << (unsigned)m_global_features.size();
    for (auto& it : m_global_features) {
        oa << it.first << (unsigned)it.second.size();
        for (auto& cloud : it.second) {
            oa << (unsigned)cloud.size();
            for (auto& f : cloud) {
                for (int r = 0; r < 9; ++r) oa << f.rf[r];
                oa << f.descriptor << f.radius << f.instanceId;
            }
        }
    }
}
bool Voting::load(BoostBinaryIArchive& ia) {
    m_dimensions_map.clear(); m_variance_map.clear();
    unsigned n = 0; ia >> n;
    if (!ia.plausible(n, 12)) return false;
    for (unsigned i = 0; i < n; ++i) { unsigned c = 0; float a = 0, b = 0; ia >> c >> a >> b; m_dimensions_map[c] = {a, b}; }
    ia >> n;
    if (!ia.plausible(n, 12)) return false;
    for (unsigned i = 0; i < n; ++i) { unsigned c = 0; float a = 0, b = 0; ia >> c >> a >> b; m_variance_map[c] = {a, b}; }
    // global features must be deserialised completely even when unused (voting.cpp:652-705); they are kept with the model
    m_global_features.clear();
    unsigned n_glob = 0; ia >> n_glob;
    if (!ia.plausible(n_glob, 8)) return false;
    for (unsigned i = 0; i < n_glob && ia.ok(); ++i) {
        unsigned classId = 0, clouds = 0; ia >> classId >> clouds;
        if (!ia.plausible(clouds, 4)) return false;
        auto& per_class = m_global_features[classId];
        for (unsigned j = 0; j < clouds && ia.ok(); ++j) {
            unsigned feats = 0; ia >> feats;
            if (!ia.plausible(feats, 52)) return false;
            per_class.emplace_back();
            for (unsigned k = 0; k < feats && ia.ok(); ++k) {
                StoredGlobalFeature f; f.classId = classId;
                for (int r = 0; r < 9; ++r) ia >> f.rf[r];
                ia >> f.descriptor >> f.radius >> f.instanceId;
                per_class.back().push_back(f);
            }
        }
    }
    return ia.ok();
}

// ---------------------------------------------------------------------------------------------------------------
// Voting (voting/voting.cpp, voting_mean_shift.cpp)
// ---------------------------------------------------------------------------------------------------------------
Voting::Voting() {                                // voting.cpp:28-50
    addParameter(m_minThreshold, "MinThreshold", 0.0f);
    addParameter(m_minVotesThreshold, "MinVotesThreshold", 1);
    addParameter(m_bestK, "BestK", -1);
    addParameter(m_averageRotation, "AverageRotation", false);
    addParameter(m_radiusType, "BinOrBandwidthType", std::string("Config"));
    addParameter(m_radiusFactor, "BinOrBandwidthFactor", 1.0f);
    addParameter(m_max_filter_type, "MaxFilterType", std::string("None"));
    addParameter(m_max_type_param, "SingleObjectMaxType", std::string("Default"));
    addParameter(m_single_object_mode, "SingleObjectMode", false);
    addParameter(m_use_global_features, "UseGlobalFeatures", false);
    addParameter(m_global_feature_method, "GlobalFeaturesStrategy", std::string("KNN"));     // voting.cpp:39-45
    addParameter(m_k_global_features, "GlobalFeaturesK", 1);
    addParameter(m_merge_function, "GlobalFeatureInfluenceType", 3);
    addParameter(m_min_svm_score, "GlobalParamMinSvmScore", 0.70f);
    addParameter(m_rate_limit, "GlobalParamRateLimit", 0.60f);
    addParameter(m_weight_factor, "GlobalParamWeightFactor", 1.5f);
    addParameter(m_min_points, "GlobalFeatureMinPoints", 500);
    addParameter(m_vote_filtering_with_ransac, "RansacVoteFiltering", false);      // voting.cpp:47-50
    addParameter(m_refine_model, "RansacRefineModel", false);
    addParameter(m_inlier_threshold, "RansacInlierThreshold", 0.1f);
    addParameter(m_inlier_threshold_type, "RansacInlierThresholdType", std::string("Fixed"));
}
// Voting::findMaxima (voting.cpp:112-122): the threshold of every class; "ObjectRadius" / "BoundingBoxMedian" scale it by the class's
// entry of m_dimensions_map, anything else is "Fixed". Resolved per class like BinOrBandwidthType (searchDistPerClass).
std::vector<float> Voting::ransacThresholdPerClass(int n_classes) const {
    const bool first = m_inlier_threshold_type == "ObjectRadius", second = m_inlier_threshold_type == "BoundingBoxMedian";
    if (!first && !second) return {};
    std::vector<float> out((size_t)n_classes, m_inlier_threshold);
    for (int c = 0; c < n_classes; ++c) {
        auto it = m_dimensions_map.find((unsigned)c);
        if (it == m_dimensions_map.end()) continue;            // a class that was never trained casts no votes either
        out[c] = m_inlier_threshold * (first ? it->second.first : it->second.second);
    }
    return out;
}
void Voting::fillRansacParams(DeviceSession& s, const std::vector<float>& class_thr, ismhip_ransac_params& R) const {
    R.vote_keypoint = s.v_kp.as<float>(); R.vote_keypoint_training = s.v_kpt.as<float>();
    R.inlier_threshold = m_inlier_threshold; R.class_inlier_threshold_h = class_thr.empty() ? nullptr : class_thr.data();
    R.max_iterations = 10000;                                  // corr_rejector.setMaximumIterations(10000) (voting.cpp:398)
    R.seed = 12345ull;                                         // PCL seeds every cluster's generator with 12345; the draws are this library's
}
void Voting::clear() {}
std::vector<std::vector<VotingMaximum>> Voting::findMaxima(DeviceSession& s, int metric) {
    if (m_max_filter_type != "None" && m_max_filter_type != "Simple" && m_max_filter_type != "Merge")
        LOG_ERROR("Invalid maxima filter type specified: " << m_max_filter_type << "! No filtering is performed!");            // maxima_handler.cpp:292-295
    if (m_max_type_param != "None" && m_max_type_param != "Default" && m_max_type_param != "BandwidthVotes" && m_max_type_param != "VotingSpaceVotes" &&
        m_max_type_param != "ModelRadiusVotes")
        LOG_WARN("Invalid single object maximum type: " << m_max_type_param << "! Using default instead.");                   // maxima_handler.h:53-57
    std::vector<std::vector<VotingMaximum>> out(s.n_obj);
    if (s.n_slots == 0) {                                      // no vote in the whole batch: no maxima; the global step may still speak
        if (m_use_global_features) verifyWithGlobalFeatures(s, metric, out);
        return out;
    }
    if (singleObjectMaxType() != ISMHIP_SOM_MEANSHIFT) {       // voting_mean_shift.cpp:124-157: the query point is the centroid of the object's cloud
        s.obj_cen.reserve((size_t)s.n_obj * 12); s.obj_rad.reserve((size_t)s.n_obj * 4);
        s.check(ismhip_cloud_centroids(s.ctx, s.cloud, s.obj_cen.as<float>()), "ismhip_cloud_centroids");
        s.check(ismhip_cloud_radii(s.ctx, s.cloud, s.obj_cen.as<float>(), s.obj_rad.as<float>()), "ismhip_cloud_radii");
    }
    iFindMaxima(s, out);
    if (m_use_global_features) verifyWithGlobalFeatures(s, metric, out);
    return out;
}
// Utils::computeMVBB (utils.cpp:242-293) of regions of a search surface (ismhip_region_mvbb): position in the world, size, and rotQuat =
// matrix2Quat of the matrix whose COLUMNS are the axes (:275-287), which that function reads as memory rows: hostRotQuaternion of the
// axes rows. quatRotateInv (:290) of the centre in box coordinates is then the world centre the device returns.
static std::vector<BoundingBox> regionMVBBs(DeviceSession& s, const ismhip_cloud* cloud, const std::vector<int32_t>& r_obj, const std::vector<float>& r_cen,
                                            const std::vector<float>& r_rad, std::vector<uint32_t>* n_sel_out = nullptr) {
    const size_t R = r_obj.size();
    std::vector<BoundingBox> boxes(R);
    if (R == 0) return boxes;
    DevBuf obj, cen, rad, n_sel, center, size, axes;
    DeviceSession::h2d(obj, r_obj); DeviceSession::h2d(cen, r_cen); DeviceSession::h2d(rad, r_rad);
    n_sel.reserve(R * 4); center.reserve(R * 12); size.reserve(R * 12); axes.reserve(R * 36);
    s.check(ismhip_region_mvbb(s.ctx, cloud, (int)R, obj.as<int32_t>(), cen.as<float>(), rad.as<float>(), n_sel.as<uint32_t>(), center.as<float>(),
                               size.as<float>(), axes.as<float>(), nullptr, nullptr), "ismhip_region_mvbb");
    std::vector<uint32_t> hn; std::vector<float> hc, hs, ha;
    s.d2h(hn, n_sel, R); s.d2h(hc, center, R * 3); s.d2h(hs, size, R * 3); s.d2h(ha, axes, R * 9);
    for (size_t r = 0; r < R; ++r) {
        if (hn[r] == 0) continue;                             // nothing selected: the default box
        for (int d = 0; d < 3; ++d) { boxes[r].position[d] = hc[r * 3 + d]; boxes[r].size[d] = hs[r * 3 + d]; }
        hostRotQuaternion(&ha[r * 9], boxes[r].rotQuat.data());
    }
    if (n_sel_out) *n_sel_out = hn;
    return boxes;
}
// The global step of Voting::findMaxima (voting.cpp:217-298) for a whole batch: one region per object (single-object mode) or per
// maximum (its position, the class's median box edge as radius: global_radii, voting.cpp:634), ALL regions in one device call, one exact
// kNN call on the stored training rows, then classifyWithKNN and the merge sequence on the host.
void Voting::verifyWithGlobalFeatures(DeviceSession& s, int metric, std::vector<std::vector<VotingMaximum>>& out) {
    if (!m_global_descriptor) throw RuntimeException("UseGlobalFeatures needs a built GlobalFeatures type (built: " + std::string(GlobalFeatures::builtTypes()) + ")");
    // the stored rows in the order the reference concatenates them (voting.cpp:660-701): class, cloud, row
    std::vector<float> rows; std::vector<unsigned> row_class, row_inst;
    const int D = m_global_descriptor->getDescriptorLength();
    for (auto& it : m_global_features) for (auto& cloud : it.second) for (auto& f : cloud) {
        if ((int)f.descriptor.size() != D)
            throw RuntimeException("the model's stored global features have " + std::to_string(f.descriptor.size()) + " dimensions, the configured GlobalFeatures type " + std::to_string(D));
        rows.insert(rows.end(), f.descriptor.begin(), f.descriptor.end()); row_class.push_back(it.first); row_inst.push_back(f.instanceId);
    }
    const int n_rows = (int)row_class.size();
    if (n_rows == 0) throw RuntimeException("UseGlobalFeatures: the model holds no global features (train it with a built GlobalFeatures type)");
    const int K = std::min(std::max(m_k_global_features, 1), n_rows);                // FLANN returns what there is: clamp to the stored rows
    if (K > ISMHIP_KNN_LARGE_K_MAX) throw RuntimeException("GlobalFeaturesK " + std::to_string(K) + " is not built (ismhip_knn_large_k: up to " + std::to_string(ISMHIP_KNN_LARGE_K_MAX) + ")");
    if (D > ISMHIP_SHORT_CSHOT_MAX_DIM) throw RuntimeException("global descriptor length " + std::to_string(D) + " is not built (ismhip_knn: up to " + std::to_string(ISMHIP_SHORT_CSHOT_MAX_DIM) + ")");
    // regions
    std::vector<int32_t> r_obj, r_max; std::vector<float> r_cen, r_rad;
    for (int o = 0; o < s.n_obj; ++o) {
        if (m_single_object_mode) { r_obj.push_back(o); r_max.push_back(-1); r_cen.insert(r_cen.end(), 3, 0.f); r_rad.push_back(-1.f); continue; }
        for (size_t i = 0; i < out[o].size(); ++i) {
            const VotingMaximum& m = out[o][i];
            auto dim = m_dimensions_map.find(m.classId);
            r_obj.push_back(o); r_max.push_back((int32_t)i);
            r_cen.insert(r_cen.end(), m.position.begin(), m.position.end());
            r_rad.push_back(dim == m_dimensions_map.end() ? 0.f : dim->second.second);      // a class without dimensions selects nothing
        }
    }
    GlobalDump dump; dump.k = K; dump.dim = D; dump.region_obj = r_obj; dump.region_max = r_max;
    dump.max_off.assign(1, 0u);
    for (int o = 0; o < s.n_obj; ++o) {
        for (const VotingMaximum& m : out[o]) {
            dump.max_cls.push_back((int32_t)m.classId); dump.max_inst.push_back((int32_t)m.instanceId); dump.max_w.push_back(m.weight); dump.max_iw.push_back(m.instanceWeight);
            dump.max_pos.insert(dump.max_pos.end(), m.position.begin(), m.position.end());
        }
        dump.max_off.push_back((uint32_t)dump.max_cls.size());
    }
    const int R = (int)r_obj.size();
    std::vector<VotingMaximum::GlobalHypothesis> hyp((size_t)R);
    if (R > 0) {
        GlobalRegions G; G.set(r_obj, r_cen, r_rad, D);
        m_global_descriptor->describe(s, G);
        std::vector<float> desc;
        const size_t T = G.rows();                                                   // query rows: one per region, but for CVFH (G.row_off)
        dump.row_off = G.row_off;
        s.d2h(dump.n_sel, G.n_sel, (size_t)R); s.d2h(dump.centroid, G.centroid, (size_t)R * 3); s.d2h(dump.radius, G.radius, (size_t)R);
        if (T > 0) s.d2h(desc, G.desc, T * D);
        dump.desc = desc;
        // which rows are searched: their region has enough points (classify(), global_classifier.cpp:181; single-object mode passes -1)
        // and the row is not NaN. A region without such a row gets the zero-weight hypothesis of :229-239; a row that is not searched is
        // zeroed so that the search sees no NaN.
        std::vector<uint8_t> live(T, 0);
        for (int r = 0; r < R; ++r) {
            const bool enough = m_single_object_mode || (int)dump.n_sel[r] > m_min_points || m_min_points < 0;
            for (size_t t = G.row_off[r]; t < G.row_off[r + 1]; ++t) {
                live[t] = enough && !std::isnan(desc[t * D]);
                if (!live[t]) std::fill(desc.begin() + t * D, desc.begin() + (t + 1) * D, 0.f);
            }
        }
        if (T > 0) {                                                                 // ALL rows of all regions: one search
            DevBuf q, idx, dist;
            DeviceSession::h2d(q, desc);
            idx.reserve(T * K * 4); dist.reserve(T * K * 4);
            const TempCodebook cb = searchOnlyCodebook(s, (uint32_t)n_rows, D, rows.data());
            if (K <= 16) s.check(ismhip_knn(s.ctx, cb.get(), metric, (int)T, q.as<float>(), K, idx.as<int32_t>(), dist.as<float>()), "ismhip_knn (global features)");
            else s.check(ismhip_knn_large_k(s.ctx, cb.get(), metric, (int)T, q.as<float>(), K, idx.as<int32_t>(), dist.as<float>()), "ismhip_knn_large_k (global features)");
            s.d2h(dump.knn_idx, idx, T * K); s.d2h(dump.knn_dist, dist, T * K);
        }
        for (int r = 0; r < R; ++r) {
            const VotingMaximum* m = r_max[r] >= 0 ? &out[r_obj[r]][r_max[r]] : nullptr;
            VotingMaximum::GlobalHypothesis g;
            g.classId = m ? m->classId : (unsigned)-1; g.instanceId = m ? m->instanceId : (unsigned)-1;      // the zero-weight hypothesis
            // the neighbours of the region's live rows, row after row (the loop of global_classifier.cpp:249-284 feeds one accumulator)
            std::vector<unsigned> nc, ni; std::vector<float> nd;
            for (size_t t = G.row_off[r]; t < G.row_off[r + 1]; ++t) {
                if (!live[t]) continue;
                for (int j = 0; j < K; ++j) {
                    const int32_t w = dump.knn_idx[t * K + j];
                    nc.push_back(row_class[w]); ni.push_back(row_inst[w]); nd.push_back(dump.knn_dist[t * K + j]);
                }
            }
            if (!nc.empty()) g = classifyWithKNN((int)nc.size(), nc.data(), ni.data(), nd.data(), g.classId, m_single_object_mode);
            hyp[r] = g;
            dump.hyp_id.push_back(g.classId); dump.hyp_id.push_back(g.instanceId); dump.hyp_w.push_back(g.classWeight); dump.hyp_w.push_back(g.instanceWeight);
        }
    }
    // hypotheses onto the maxima
    std::vector<int> boxless;                                                        // single-object mode: regions of objects without maxima
    for (int r = 0; r < R; ++r) {
        const int o = r_obj[r];
        if (!m_single_object_mode) {
            VotingMaximum& m = out[o][r_max[r]];
            m.globalHypothesis = hyp[r];
            if (dump.n_sel[r] > 0) m.roiCentroid = {dump.centroid[(size_t)r * 3], dump.centroid[(size_t)r * 3 + 1], dump.centroid[(size_t)r * 3 + 2]};
            continue;
        }
        for (VotingMaximum& m : out[o]) m.globalHypothesis = hyp[r];                 // voting.cpp:246-247
        if (out[o].empty() && dump.n_sel[r] > 0) boxless.push_back(r);                // :250-260
    }
    dump.box.assign((size_t)R * 10, std::numeric_limits<float>::quiet_NaN());
    if (!boxless.empty()) {                                                          // their boxes: Utils::computeMVBB of the region (:258), one call
        std::vector<int32_t> b_obj; std::vector<float> b_cen, b_rad;
        for (int r : boxless) { b_obj.push_back(r_obj[r]); b_cen.insert(b_cen.end(), r_cen.begin() + (size_t)r * 3, r_cen.begin() + (size_t)r * 3 + 3); b_rad.push_back(r_rad[r]); }
        const std::vector<BoundingBox> boxes = regionMVBBs(s, s.cloud, b_obj, b_cen, b_rad);
        for (size_t i = 0; i < boxless.size(); ++i) {
            const int r = boxless[i], o = r_obj[r];
            VotingMaximum m;
            m.globalHypothesis = hyp[r];
            m.classId = hyp[r].classId; m.weight = hyp[r].classWeight; m.instanceId = hyp[r].instanceId;
            m.position = {dump.centroid[(size_t)r * 3], dump.centroid[(size_t)r * 3 + 1], dump.centroid[(size_t)r * 3 + 2]};
            m.boundingBox = boxes[i];
            float* b = &dump.box[(size_t)r * 10];
            std::copy(boxes[i].position.begin(), boxes[i].position.end(), b); std::copy(boxes[i].size.begin(), boxes[i].size.end(), b + 3);
            std::copy(boxes[i].rotQuat.begin(), boxes[i].rotQuat.end(), b + 6);
            out[o].push_back(m);
        }
    }
    MergeParams P;
    P.function = m_merge_function; P.radius = mergeRadius(); P.min_threshold = m_minThreshold; P.best_k = m_bestK;
    P.min_svm_score = m_min_svm_score; P.rate_limit = m_rate_limit; P.weight_factor = m_weight_factor;
    for (int o = 0; o < s.n_obj; ++o) mergeSequence(out[o], P);
    m_last_global = dump;
}
int Voting::singleObjectMaxType() const {                      // maxima_handler.h:42-58; only consulted in single-object mode (voting_mean_shift.cpp:80)
    if (!m_single_object_mode) return ISMHIP_SOM_MEANSHIFT;
    if (m_max_type_param == "BandwidthVotes") return ISMHIP_SOM_BANDWIDTH;
    if (m_max_type_param == "VotingSpaceVotes") return ISMHIP_SOM_COMPLETE_VOTING_SPACE;
    if (m_max_type_param == "ModelRadiusVotes") return ISMHIP_SOM_MODEL_RADIUS;
    return ISMHIP_SOM_MEANSHIFT;
}
int Voting::maxFilter() const {                                // voting.cpp:262-268: no inter-class filter in single-object mode
    if (m_single_object_mode) return ISMHIP_MAXFILTER_NONE;
    return m_max_filter_type == "Simple" ? ISMHIP_MAXFILTER_SIMPLE : (m_max_filter_type == "Merge" ? ISMHIP_MAXFILTER_MERGE : ISMHIP_MAXFILTER_NONE);
}

// M = maxima per object the buffers hold. The reference returns every maximum (voting.cpp:236-272), the device call a fixed capacity:
// the host asks for 32 and, when some object fills them all, again for 1024 = the kernels' own per-object limit, beyond which
// ismhip_sync reports the truncation.
struct Voting::MaximaBuffers { DevBuf n_max, pos, w, cls, inst, iw, bs, bq, nv, score; int M = 32; void reserve(int n_obj, int C); };
// The maxima search of both back ends: P carries the back end's own fields, the fields the two parameter structs share are filled
// here; `entry` / `ransac_entry` are its plain entry point and the one with the RANSAC vote filter (two arguments more).
template <typename Params, typename Entry, typename RansacEntry>
void Voting::searchMaxima(DeviceSession& s, Params P, Entry entry, RansacEntry ransac_entry, const char* what, std::vector<std::vector<VotingMaximum>>& out) const {
    P.n_classes = std::max(1, s.n_classes);
    P.min_votes_threshold = m_minVotesThreshold; P.min_threshold = m_minThreshold; P.best_k = m_bestK;
    // with global verification the device does the first normalisation only: MinThreshold and BestK close the host's merge sequence
    if (m_use_global_features) { P.min_threshold = 0.f; P.best_k = -1; }
    P.max_filter = maxFilter();
    for (int M : {32, 1024}) {
        MaximaBuffers B; B.M = M; B.reserve(s.n_obj, P.n_classes);
        P.max_maxima = M;
        if (m_averageRotation) { P.vote_bbox_quat = s.v_bq.as<float>(); P.max_bbox_quat_out = B.bq.as<float>(); }              // voting.cpp:210-215
        auto call = [&](auto fn, auto... filter_args) {
            return fn(s.ctx, s.n_obj, s.slot_off.data(), s.v_pos.as<float>(), s.v_w.as<float>(), s.v_cls.as<int32_t>(), s.v_inst.as<int32_t>(),
                      s.v_bs.as<float>(), &P, B.n_max.as<int32_t>(), B.pos.as<float>(), B.w.as<float>(), B.cls.as<int32_t>(), B.inst.as<int32_t>(),
                      B.iw.as<float>(), B.bs.as<float>(), B.nv.as<int32_t>(), B.score.as<float>(), filter_args...);
        };
        if (m_vote_filtering_with_ransac) {                         // voting.cpp:110-127: the filter runs inside the maxima search
            const std::vector<float> class_thr = ransacThresholdPerClass(P.n_classes);
            ismhip_ransac_params R{}; fillRansacParams(s, class_thr, R);
            s.check(call(ransac_entry, &R, (float*)nullptr), (std::string(what) + "_ransac").c_str());
            s.sync();                                               // class_thr is read by the launch
        } else {
            s.check(call(entry), what);
        }
        if (collectMaxima(s, B, out, m_averageRotation)) break;     // (with 1024 slots it takes what there is)
    }
}
VotingMeanShift::VotingMeanShift() {              // voting_mean_shift.cpp:20-27
    addParameter(m_bandwidth, "Bandwidth", 0.2f);
    addParameter(m_threshold, "Threshold", 1e-3f);
    addParameter(m_maxIter, "MaxIter", 1000);
    addParameter(m_kernel, "Kernel", std::string("Gaussian"));
    addParameter(m_maxima_suppression_type, "MaximaSuppression", std::string("Average"));
}
void VotingMeanShift::iFindMaxima(DeviceSession& s, std::vector<std::vector<VotingMaximum>>& out) {
    ismhip_maxima_params P{};
    const std::vector<float> class_bw = searchDistPerClass(m_bandwidth, std::max(1, s.n_classes));      // voting_mean_shift.cpp:46-49
    P.class_bandwidth_h = class_bw.empty() ? nullptr : class_bw.data(); P.bandwidth = m_bandwidth; P.threshold = m_threshold; P.max_iter = m_maxIter;
    P.kernel = m_kernel == "Uniform" ? ISMHIP_KERNEL_UNIFORM : ISMHIP_KERNEL_GAUSSIAN;
    P.suppression = m_maxima_suppression_type == "Average" ? ISMHIP_SUPPRESS_AVERAGE : (m_maxima_suppression_type == "Suppress" ? ISMHIP_SUPPRESS_SUPPRESS : ISMHIP_SUPPRESS_NONE);
    P.single_object_max_type = singleObjectMaxType(); P.object_centroid = s.obj_cen.as<float>(); P.object_radius = s.obj_rad.as<float>();
    searchMaxima(s, P, ismhip_find_maxima, ismhip_find_maxima_ransac, "ismhip_find_maxima", out);
}
void Voting::MaximaBuffers::reserve(int n_obj, int C) {
    const size_t t = (size_t)n_obj * M;
    n_max.reserve((size_t)n_obj * 4); pos.reserve(t * 12); w.reserve(t * 4); cls.reserve(t * 4); inst.reserve(t * 4); iw.reserve(t * 4); bs.reserve(t * 12);
    nv.reserve(t * 4); score.reserve((size_t)n_obj * C * 4); bq.reserve(t * 16);
}
// returns false when some object filled all M slots (the caller asks again with more room)
bool Voting::collectMaxima(DeviceSession& s, MaximaBuffers& b, std::vector<std::vector<VotingMaximum>>& out, bool with_quat) {
    const int M = b.M; const size_t t = (size_t)s.n_obj * M;
    std::vector<int32_t> hn, hcls, hinst, hnv; std::vector<float> hpos, hw, hiw, hbs, hbq;
    s.d2h(hn, b.n_max, s.n_obj);
    for (int o = 0; o < s.n_obj; ++o) if (hn[o] >= M && M < 1024) return false;
    if (with_quat) s.d2h(hbq, b.bq, t * 4);
    s.d2h(hpos, b.pos, t * 3); s.d2h(hw, b.w, t); s.d2h(hcls, b.cls, t); s.d2h(hinst, b.inst, t); s.d2h(hiw, b.iw, t); s.d2h(hbs, b.bs, t * 3); s.d2h(hnv, b.nv, t);
    for (int o = 0; o < s.n_obj; ++o)
        for (int m = 0; m < hn[o]; ++m) {
            const size_t i = (size_t)o * M + m;
            VotingMaximum vm;
            vm.position = {hpos[i * 3], hpos[i * 3 + 1], hpos[i * 3 + 2]}; vm.weight = hw[i]; vm.classId = (unsigned)hcls[i]; vm.instanceId = (unsigned)hinst[i];
            vm.instanceWeight = hiw[i]; vm.numVotes = hnv[i];
            vm.boundingBox.position = vm.position; vm.boundingBox.size = {hbs[i * 3], hbs[i * 3 + 1], hbs[i * 3 + 2]};
            if (with_quat) vm.boundingBox.rotQuat = {hbq[i * 4], hbq[i * 4 + 1], hbq[i * 4 + 2], hbq[i * 4 + 3]};
            out[o].push_back(vm);
        }
    return true;
}

VotingHough3D::VotingHough3D() {                  // voting_hough_3d.cpp:15-26
    addParameter(m_useInterpolation, "UseInterpolation", true);
    addParameter(m_minCoord, "MinCoord", Vec3d{{-5, -5, -5}});
    addParameter(m_maxCoord, "MaxCoord", Vec3d{{5, 5, 5}});
    addParameter(m_binSize, "BinSize", Vec3d{{0.2, 0.2, 0.2}});
    addParameter(m_relThreshold, "RelThreshold", 0.8f);
}
void VotingHough3D::iFindMaxima(DeviceSession& s, std::vector<std::vector<VotingMaximum>>& out) {
    if (m_single_object_mode) LOG_WARN("SingleObjectMode is not supported with Hough3D - switch to MeanShift to use it!");   // :42-43
    ismhip_hough_params P{};
    for (int d = 0; d < 3; ++d) { P.min_coord[d] = (float)m_minCoord[d]; P.max_coord[d] = (float)m_maxCoord[d]; }
    // :45-47: MaximaHandler::setRadius(BinSize[0] / 2); the bins become cubes of edge 2 * getSearchDistForClass (= BinSize[0] with "Config")
    P.bin_size = 2.0f * (float)(m_binSize[0] / 2);
    std::vector<float> class_bin = searchDistPerClass((float)(m_binSize[0] / 2), std::max(1, s.n_classes));
    for (float& b : class_bin) b *= 2.0f;
    P.class_bin_h = class_bin.empty() ? nullptr : class_bin.data();
    P.use_interpolation = m_useInterpolation ? 1 : 0; P.rel_threshold = m_relThreshold;
    searchMaxima(s, P, ismhip_hough3d_maxima, ismhip_hough3d_maxima_ransac, "ismhip_hough3d_maxima", out);
}

// ---------------------------------------------------------------------------------------------------------------
// Factories (features_factory.h:47-110, keypoints_factory.h:24-38, activation_strategy_factory.h:22-35, voting_factory.h:20-29)
// ---------------------------------------------------------------------------------------------------------------
template <> Features* Factory<Features>::createByType(const std::string& type) {
    if (type == FeaturesSHOT::getTypeStatic()) return new FeaturesSHOT();
    if (type == FeaturesCSHOT::getTypeStatic()) return new FeaturesCSHOT();
    if (type == FeaturesFPFH::getTypeStatic()) return new FeaturesFPFH();
    if (type == FeaturesSHORTSHOT::getTypeStatic()) return new FeaturesSHORTSHOT();
    if (type == FeaturesSHORTCSHOT::getTypeStatic()) return new FeaturesSHORTCSHOT();
    if (type == FeaturesCospair::getTypeStatic()) return new FeaturesCospair();
    if (type == FeaturesBSHOT::getTypeStatic()) return new FeaturesBSHOT();
    if (type == FeaturesSpinImage::getTypeStatic()) return new FeaturesSpinImage();
    if (type == FeaturesRSD::getTypeStatic()) return new FeaturesRSD();
    if (type == FeaturesRIFT::getTypeStatic()) return new FeaturesRIFT();
    if (type == FeaturesCGF::getTypeStatic()) return new FeaturesCGF();
    if (type == FeaturesESFLocal::getTypeStatic()) return new FeaturesESFLocal();
    if (type == FeaturesUSC::getTypeStatic()) return new FeaturesUSC();
    throw RuntimeException("feature type \"" + type + "\" is outside the MI355X hot path (built: SHOT, BSHOT, CSHOT, FPFH, SHORT_SHOT, SHORT_CSHOT, ESF_LOCAL, CGF, RIFT, SpinImage, RSD, CoSPAIR) and USC");
}
template <> Keypoints* Factory<Keypoints>::createByType(const std::string& type) {
    if (type == KeypointsVoxelGrid::getTypeStatic()) return new KeypointsVoxelGrid();
    if (type == KeypointsISS3D::getTypeStatic()) return new KeypointsISS3D();
    if (type == KeypointsVoxelGridCulling::getTypeStatic()) return new KeypointsVoxelGridCulling();
    if (type == KeypointsSIFT3D::getTypeStatic()) return new KeypointsSIFT3D();
    throw RuntimeException("keypoint type \"" + type + "\" is not built (built: VoxelGrid, ISS3D, VoxelGridCulling) and SIFT3D");
}
template <> ActivationStrategy* Factory<ActivationStrategy>::createByType(const std::string& type) {
    if (type == ActivationStrategyKNN::getTypeStatic()) return new ActivationStrategyKNN();
    if (type == ActivationStrategyKnnRule::getTypeStatic()) return new ActivationStrategyKnnRule();
    if (type == ActivationStrategyThreshold::getTypeStatic()) return new ActivationStrategyThreshold();
    throw RuntimeException("activation strategy \"" + type + "\" is not built (built: KNN, KNNRule, Threshold)");
}
template <> Voting* Factory<Voting>::createByType(const std::string& type) {
    if (type == VotingMeanShift::getTypeStatic()) return new VotingMeanShift();
    if (type == VotingHough3D::getTypeStatic()) return new VotingHough3D();
    throw RuntimeException("voting type \"" + type + "\" is not built (built: MeanShift, Hough3D)");
}
template <> Codebook* Factory<Codebook>::createByType(const std::string&) { return new Codebook(); }
template <> Clustering* Factory<Clustering>::createByType(const std::string& type) {       // clustering_factory.h
    if (type == ClusteringNone::getTypeStatic()) return new ClusteringNone();
    if (type == ClusteringKMeansCount::getTypeStatic()) return new ClusteringKMeansCount();
    if (type == ClusteringKMeansFactor::getTypeStatic()) return new ClusteringKMeansFactor();
    if (type == ClusteringKMeansThumbRule::getTypeStatic()) return new ClusteringKMeansThumbRule();
    if (type == ClusteringKMeansHartigan::getTypeStatic()) return new ClusteringKMeansHartigan();
    throw RuntimeException("clustering type \"" + type + "\" is not built (built: None, KMeansCount, KMeansFactor, KMeansThumbRule, KMeansHartigan)");
}

template <> FeatureRanking* Factory<FeatureRanking>::createByType(const std::string& type) {    // ranking_factory.h
    if (type == RankingUniform::getTypeStatic()) return new RankingUniform();
    if (type == RankingKnnActivation::getTypeStatic()) return new RankingKnnActivation();
    if (type == RankingIncremental::getTypeStatic()) return new RankingIncremental();
    if (type == RankingStrangeness::getTypeStatic()) return new RankingStrangeness();
    if (type == RankingNaiveBayes::getTypeStatic()) return new RankingNaiveBayes();
    throw RuntimeException("feature ranking type \"" + type + "\" is not built (built: Uniform, KNNActivation, Incremental, Strangeness, NaiveBayes)");
}

// ---------------------------------------------------------------------------------------------------------------
// FeatureRanking (feature_ranking/*.cpp): scores and selection run on the device (ismhip_rank_scores, ismhip_rank_select)
// ---------------------------------------------------------------------------------------------------------------
FeatureRanking::FeatureRanking() {                 // feature_ranking.cpp:21-29
    addParameter(m_k_search, "KSearch", 10);
    addParameter(m_dist_thresh, "DistanceThreshold", 0.1f);
    addParameter(m_factor, "Factor", 0.75f);
    addParameter(m_extract_list, "ExtractFromList", std::string("invalid"));
    addParameter(m_extract_offset, "ExtractOffset", 0.0f);
}
void FeatureRanking::iPostInitConfig() {           // :135-148, applied when the configuration is read instead of at the first ranking
    if (m_extract_list == "invalid") return;
    LOG_WARN("Config parameter \"ExtractFromList\" is deprecated. Use \"ExtractOffset\" instead!");
    LOG_WARN("For now, the given value for \"ExtractFromList\" will be automatically converted.");
    if (m_extract_list == "front") m_extract_offset = 0.0f;
    if (m_extract_list == "center" || m_extract_list == "middle") m_extract_offset = 0.5 * (1 - m_factor);
    if (m_extract_list == "back") m_extract_offset = 1.0 - m_factor;
}
RankingKnnActivation::RankingKnnActivation() {     // ranking_knn_activation.cpp:15-19
    addParameter(m_use_feature_position, "UseFeaturePosition", false);
    addParameter(m_score_increment_type, "ScoreIncrementType", 0);
}
void RankingKnnActivation::iPostInitConfig() {
    FeatureRanking::iPostInitConfig();
    if (m_use_feature_position)
        throw RuntimeException("feature ranking KNNActivation with UseFeaturePosition true is not built: the training batch carries no centerDist "
                               "(built: Uniform, KNNActivation without UseFeaturePosition, Incremental, Strangeness, NaiveBayes)");
}
int RankingKnnActivation::incrementType() {        // :88-95
    m_score_increment_type = m_score_increment_type == 0 ? 1 : m_score_increment_type;
    if (m_score_increment_type > 3 || m_score_increment_type < 1) {
        LOG_WARN("Invalid score increment type: " << m_score_increment_type << "! Using type 1 instead.");
        m_score_increment_type = 1;
    }
    return m_score_increment_type;
}
std::vector<uint8_t> FeatureRanking::operator()(DeviceSession& s, const DeviceFeatures& f, const std::vector<uint32_t>& class_offsets) {
    std::vector<uint8_t> mask;
    if (f.n == 0 || class_offsets.size() < 2) return mask;
    const int n_classes = (int)class_offsets.size() - 1;
    LOG_INFO("starting " << getType() << " ranking");
    if (m_k_search < 1) throw BadParamExceptionType<int>("invalid feature ranking KSearch", m_k_search);
    DevBuf score, keep;
    score.reserve((size_t)f.n * 4); keep.reserve(f.n);
    s.check(ismhip_rank_scores(s.ctx, deviceType(), (int)f.n, f.dim, f.desc.as<float>(), n_classes, class_offsets.data(), m_k_search, m_dist_thresh,
                               incrementType(), score.as<float>()), "ismhip_rank_scores");
    std::vector<uint32_t> n_keep((size_t)n_classes, 0u);
    s.check(ismhip_rank_select(s.ctx, (int)f.n, n_classes, class_offsets.data(), score.as<float>(), m_factor, m_extract_offset, keep.as<uint8_t>(),
                               n_keep.data()), "ismhip_rank_select");
    s.d2h(mask, keep, f.n);
    size_t kept = 0;
    for (uint32_t k : n_keep) kept += k;
    LOG_INFO("input features: " << f.n << ", output features: " << kept << ", output ratio: " << (((float)kept) / (f.n)));   // :113-115
    return mask;
}

// ---------------------------------------------------------------------------------------------------------------
// Clustering (clustering/*.cpp): k-means runs on the device (ismhip_kmeans)
// ---------------------------------------------------------------------------------------------------------------
struct ClusterCenters { DevBuf buf; };
Clustering::Clustering() {}
Clustering::~Clustering() {}
void Clustering::clear() { m_n_centers = 0; m_indices.clear(); m_distances.clear(); }
const float* Clustering::getClusterCentersDevice() const { return m_centers ? m_centers->buf.as<float>() : nullptr; }
void ClusteringNone::process(DeviceSession&, const DeviceFeatures& f, int) {
    m_indices.resize(f.n);
    std::iota(m_indices.begin(), m_indices.end(), 0);
}
ClusteringKMeans::ClusteringKMeans() {             // clustering_kmeans.cpp:18-26
    addParameter(m_iterations, "Iterations", 1000);
    addParameter(m_centersInit, "CentersInit", std::string("FLANN_CENTERS_KMEANSPP"));
    addParameter(m_cbIndex, "CbIndex", 0.5f);      // FLANN's cluster-boundary index: search-time only, without effect on the exact search here
    addParameter(m_seed, "Seed", 0);               // this build's random draws (the reference draws from rand())
}
void ClusteringKMeans::cluster(DeviceSession& s, const DeviceFeatures& f, int metric, int clusterCount) {   // clustering_kmeans.cpp:32-52, .h:53-131
    if (f.n == 0) return;
    if (clusterCount == 0) clusterCount = 1;
    int init;
    if (m_centersInit == "FLANN_CENTERS_RANDOM") init = ISMHIP_CENTERS_RANDOM;
    else if (m_centersInit == "FLANN_CENTERS_GONZALES") init = ISMHIP_CENTERS_GONZALES;
    else if (m_centersInit == "FLANN_CENTERS_KMEANSPP") init = ISMHIP_CENTERS_KMEANSPP;
    else throw BadParamExceptionType<std::string>("invalid flann centers init", m_centersInit);
    if (clusterCount > (int)f.n) {
        LOG_WARN("Desired clusters is higher than available feature count. Creating " << f.n << " individual clusters.");
        clusterCount = (int)f.n;
    }
    LOG_INFO("clustering " << f.n << " features into " << clusterCount << " clusters");
    if (metric != ISMHIP_METRIC_L2SQ)
        LOG_WARN("The k-means algorithm is only defined on euclidean distance. Using other distance metrics may lead to unexpected results.");
    if (!m_centers) m_centers.reset(new ClusterCenters());
    m_centers->buf.reserve((size_t)clusterCount * f.dim * sizeof(float));
    DevBuf assign, dist;
    assign.reserve((size_t)f.n * 4); dist.reserve((size_t)f.n * 4);
    int32_t count = 0, iters = 0;
    s.check(ismhip_kmeans(s.ctx, metric, (int)f.n, f.dim, f.desc.as<float>(), clusterCount, m_iterations, init, (unsigned long long)(long long)m_seed,
                          m_centers->buf.as<float>(), assign.as<int32_t>(), dist.as<float>(), &count, &iters), "ismhip_kmeans");
    if (count != clusterCount) LOG_WARN("Requested " << clusterCount << " but extracted " << count << " clusters instead");
    LOG_INFO("k-means: " << iters << " iterations");
    m_n_centers = count;
    std::vector<int32_t> idx; s.d2h(idx, assign, f.n);
    m_indices.assign(idx.begin(), idx.end());
    s.d2h(m_distances, dist, f.n);
}
ClusteringKMeansCount::ClusteringKMeansCount() { addParameter(m_clusterCount, "ClusterCount", 10); }
void ClusteringKMeansCount::process(DeviceSession& s, const DeviceFeatures& f, int metric) { cluster(s, f, metric, m_clusterCount); }
ClusteringKMeansFactor::ClusteringKMeansFactor() { addParameter(m_clusterFactor, "ClusterFactor", 0.2f); }
void ClusteringKMeansFactor::process(DeviceSession& s, const DeviceFeatures& f, int metric) {
    if (m_clusterFactor > 1) { LOG_WARN("cluster count factor has to be in range [0, 1], setting to 0.5"); m_clusterFactor = 0.5f; }
    cluster(s, f, metric, (int)std::round(f.n * m_clusterFactor));
}
void ClusteringKMeansThumbRule::process(DeviceSession& s, const DeviceFeatures& f, int metric) {
    cluster(s, f, metric, (int)std::round(std::sqrt(f.n / 2.0f)));     // Mardia, Multivariate Analysis, p. 365
}
ClusteringKMeansHartigan::ClusteringKMeansHartigan() { addParameter(m_maxK, "MaxK", 10); }
void ClusteringKMeansHartigan::process(DeviceSession& s, const DeviceFeatures& f, int metric) {   // clustering_kmeans_hartigan.cpp:27-66
    const int maxK = std::max(1, m_maxK);
    std::vector<float> dispersions(maxK);
    for (int i = 0; i < maxK; ++i) {
        cluster(s, f, metric, i + 1);
        float compactness = 0.0f;                   // withinClusterSumOfSquares: distance of every feature to its nearest centre
        for (float d : m_distances) compactness += d;
        dispersions[i] = compactness;
    }
    int bestK = 0; float maxValue = 0;
    for (int i = 0; i + 1 < maxK; ++i) {
        const int numClusters = i + 1;
        const float factor = (float)((int)f.n - numClusters - 1);
        const float index = ((dispersions[i] / dispersions[i + 1]) - 1) * factor;
        if (index > maxValue) { maxValue = index; bestK = i + 1; }
    }
    if (bestK < 1) bestK = 1;                       // the reference would index centers[-1] here
    LOG_INFO("best value for k: " << bestK);
    cluster(s, f, metric, bestK);                   // same seed, same data: the clustering of that pass again
}

// ---------------------------------------------------------------------------------------------------------------
// ImplicitShapeModel (implicit_shape_model.cpp)
// ---------------------------------------------------------------------------------------------------------------
ImplicitShapeModel::ImplicitShapeModel() {        // :91-168 (hot-path subset + the pre-filters; smoothing and voxel filtering must stay off)
    addParameter(m_distanceType, "DistanceType", std::string("Euclidean"));
    addParameter(m_normal_radius, "NormalRadius", 0.05f);
    addParameter(m_consistent_normals_method, "ConsistentNormalsMethod", 2);
    addParameter(m_num_threads, "NumThreads", 0);
    addParameter(m_bounding_box_type, "BoundingBoxType", std::string("MVBB"));
    addParameter(m_num_kd_trees, "FLANNNumKDTrees", 4);
    addParameter(m_flann_exact_match, "FLANNExactMatch", false);
    addParameter(m_instance_labels_primary, "InstanceLabelsPrimary", true);
    addParameter(m_single_object_mode_legacy, "SingleObjectMode", false);
    addParameter(m_use_smoothing, "UseSmoothing", false);
    addParameter(m_use_sor, "UseStatisticalOutlierRemoval", false);     // :95-103
    addParameter(m_sor_mean_k, "OutlierRemovalMeanK", 20);
    addParameter(m_sor_stddev_mul, "OutlierRemovalStddevMul", 2.0f);
    addParameter(m_use_ror, "UseRadiusOutlierRemoval", false);
    addParameter(m_ror_min_neighbors, "OutlierRemovalMinNeighbors", 10);
    addParameter(m_ror_radius, "OutlierRemovalRadius", 0.005f);
    addParameter(m_use_voxel_filtering, "UseVoxelFiltering", false);
    addParameter(m_cutoff_distance_z, "CutoffDistanceZAxis", 0.0f);
    m_codebook.reset(new Codebook());
    m_keypoints_detector.reset(new KeypointsVoxelGrid());
    m_feature_descriptor.reset(new FeaturesSHOT());
    m_voting.reset(new VotingMeanShift());
}
ImplicitShapeModel::~ImplicitShapeModel() {
    m_codebook.reset();     // releases its device handle while the session is alive
    m_session.reset();
}
void ImplicitShapeModel::iPostInitConfig() {      // :1260-1273
    if (m_distanceType != "Euclidean" && m_distanceType != "ChiSquared") throw BadParamExceptionType<std::string>("invalid distance type", m_distanceType);
    if (!m_flann_exact_match)
        LOG_WARN("FLANNExactMatch is false: the MI355X path always searches exactly (FLANN's randomized kd-forest with 128 checks is not reproduced)");
}
void ImplicitShapeModel::clear() { m_training_clouds.clear(); m_training_instances.clear(); }

Json ImplicitShapeModel::iChildConfigsToJson() const {   // :1070-1083
    Json c = Json::object();
    c["Codebook"] = m_codebook->configToJson();
    c["Keypoints"] = m_keypoints_detector->configToJson();
    c["Features"] = m_feature_descriptor->configToJson();
    if (!m_global_features_cfg.isNull()) c["GlobalFeatures"] = m_global_features_cfg;
    c["Clustering"] = m_clustering ? m_clustering->configToJson() : Json::parse("{\"Type\":\"None\"}");
    c["Voting"] = m_voting->configToJson();
    c["FeatureWeighting"] = m_feature_ranking ? m_feature_ranking->configToJson() : Json::parse("{\"Type\":\"Uniform\"}");
    return c;
}
bool ImplicitShapeModel::iChildConfigsFromJson(const Json& c) {   // :1085-1142
    const Json* cb = c.find("Codebook"); const Json* kp = c.find("Keypoints"); const Json* ft = c.find("Features");
    const Json* cl = c.find("Clustering"); const Json* vo = c.find("Voting"); const Json* fw = c.find("FeatureWeighting");
    if (!cb || !kp || !ft || !cl || !vo || !fw) { LOG_ERROR("missing child section (Codebook, Keypoints, Features, Clustering, Voting, FeatureWeighting are required)"); return false; }
    m_codebook.reset(Factory<Codebook>::create(*cb));
    m_keypoints_detector.reset(Factory<Keypoints>::create(*kp));
    m_feature_descriptor.reset(Factory<Features>::create(*ft));
    m_voting.reset(Factory<Voting>::create(*vo));
    if (m_voting && m_voting->refineModelRequested())
        throw RuntimeException("Voting.RansacRefineModel is not built (PCL's sac.refineModel is not restated); RansacVoteFiltering runs without it");
    m_clustering.reset(Factory<Clustering>::create(*cl));
    m_feature_ranking.reset(Factory<FeatureRanking>::create(*fw));
    if (const Json* gf = c.find("GlobalFeatures")) m_global_features_cfg = *gf;
    // the GlobalFeatures child: an object for the built types, the JSON carried through for every other one (an absent child is the
    // reference's Dummy); what is not built is refused by name, but only when the configuration asks for global verification
    m_global_descriptor.reset(GlobalFeatures::createIfBuilt(m_global_features_cfg));
    if (m_voting && m_voting->useGlobalFeatures()) {
        if (m_voting->globalStrategy() != "KNN")
            throw RuntimeException("Voting.GlobalFeaturesStrategy \"" + m_voting->globalStrategy() + "\" is not built (built: KNN; the reference's SVM needs OpenCV and is not downgraded to KNN)");
        if (!m_global_descriptor) {
            const Json* t = m_global_features_cfg.isObject() ? m_global_features_cfg.find("Type") : nullptr;
            const std::string type = t && t->type == Json::String ? t->str : std::string("Dummy");
            throw RuntimeException("Voting.UseGlobalFeatures with GlobalFeatures type \"" + type + "\" is not built (built: " + GlobalFeatures::builtTypes() + ")");
        }
    }
    if (m_voting) m_voting->setGlobalFeatureDescriptor(m_global_descriptor.get());
    // rows longer than ISMHIP_SHORT_CSHOT_MAX_DIM (USC, 1960 floats) are served by ismhip_knn up to K = 16, ismhip_train_activate and
    // ismhip_kmeans only (ISMHIP_KNN_MAX_DIM); the radius search, the large-K search and the ranking scores keep the shorter limit
    if (m_feature_descriptor && m_feature_descriptor->getDescriptorLength() > ISMHIP_SHORT_CSHOT_MAX_DIM) {
        const std::string ft_type = m_feature_descriptor->getType(), len = std::to_string(m_feature_descriptor->getDescriptorLength());
        const ActivationStrategy* as = m_codebook ? m_codebook->getActivationStrategy() : nullptr;
        if (as && as->getType() == ActivationStrategyThreshold::getTypeStatic())
            throw RuntimeException("ActivationStrategy \"Threshold\" with Features type \"" + ft_type + "\" is not built (ismhip_knn_threshold takes rows up to " +
                                   std::to_string(ISMHIP_SHORT_CSHOT_MAX_DIM) + " floats, " + ft_type + " has " + len + ")");
        if (as && as->getK() > 16)
            throw RuntimeException("ActivationStrategy K " + std::to_string(as->getK()) + " with Features type \"" + ft_type + "\" is not built (rows of " + len +
                                   " floats are searched up to K = 16)");
        if (m_feature_ranking && m_feature_ranking->ranks())
            throw RuntimeException("FeatureWeighting \"" + m_feature_ranking->getType() + "\" with Features type \"" + ft_type + "\" is not built (ismhip_rank_scores takes rows up to " +
                                   std::to_string(ISMHIP_SHORT_CSHOT_MAX_DIM) + " floats; built: Uniform)");
    }
    if (m_use_smoothing || m_use_voxel_filtering) throw RuntimeException("point cloud pre-filters smoothing (UseSmoothing) and voxel filtering (UseVoxelFiltering) are not built");
    if (m_use_sor && (m_sor_mean_k < 1 || m_sor_mean_k > ISMHIP_SOR_MAX_MEAN_K))
        throw RuntimeException("OutlierRemovalMeanK " + std::to_string(m_sor_mean_k) + " is not built (built: 1 .. " + std::to_string(ISMHIP_SOR_MAX_MEAN_K) + ")");
    if (m_use_ror && !(m_ror_radius > 0.f)) throw BadParamExceptionType<float>("invalid outlier removal radius", m_ror_radius);
    return m_codebook && m_keypoints_detector && m_feature_descriptor && m_voting && m_clustering && m_feature_ranking;
}

void ImplicitShapeModel::iSaveData(std::ostream& os) const {      // :1144-1179, as a Boost binary archive (boost_archive.h)
    BoostBinaryOArchive oa(os);
    oa << (unsigned)m_instance_to_class_map.size();
    for (auto& kv : m_instance_to_class_map) oa << kv.first << kv.second;
    m_codebook->save(oa);
    // keypoints, features, global features, clustering: JSONObject::iSaveData writes nothing (json_object.cpp:256-259)
    m_voting->save(oa);
    // feature ranking: nothing
    oa << (unsigned)m_class_labels.size();
    for (auto& kv : m_class_labels) oa << kv.second;
    oa << (unsigned)m_instance_labels.size();
    for (auto& kv : m_instance_labels) oa << kv.second;
}
bool ImplicitShapeModel::iLoadData(std::istream& is) {            // :1181-1237
    BoostBinaryIArchive ia(is);
    if (!ia.ok()) { LOG_ERROR("could not read the data file: " << ia.error()); return false; }
    unsigned size = 0; ia >> size;
    if (!ia.plausible(size, 8)) { LOG_ERROR("could not read the data file: " << ia.error()); return false; }
    m_instance_to_class_map.clear();
    for (unsigned i = 0; i < size; ++i) { unsigned a = 0, b = 0; ia >> a >> b; m_instance_to_class_map.insert({a, b}); }
    if (!m_codebook->load(ia) || !m_voting->load(ia)) { LOG_ERROR("could not load child objects: " << ia.error()); return false; }
    m_n_classes = (int)m_codebook->data().class_sigma.size();
    ia >> size;
    if (!ia.plausible(size, 8)) { LOG_ERROR("could not read the data file: " << ia.error()); return false; }
    m_class_labels.clear();
    for (unsigned i = 0; i < size; ++i) { std::string l; ia >> l; m_class_labels.insert({i, l}); }
    ia >> size;
    if (!ia.plausible(size, 8)) { LOG_ERROR("could not read the data file: " << ia.error()); return false; }
    m_instance_labels.clear();
    for (unsigned i = 0; i < size; ++i) { std::string l; ia >> l; m_instance_labels.insert({i, l}); }
    if (!ia.ok()) { LOG_ERROR("could not read the data file: " << ia.error()); return false; }
    return true;
}

bool ImplicitShapeModel::getDimensions(unsigned class_id, float* out4) const {
    auto it = m_voting->getDimensionsMap().find(class_id);
    auto iv = m_voting->getVarianceMap().find(class_id);
    if (it == m_voting->getDimensionsMap().end() || iv == m_voting->getVarianceMap().end()) return false;
    out4[0] = it->second.first; out4[1] = it->second.second; out4[2] = iv->second.first; out4[3] = iv->second.second;
    return true;
}
void ImplicitShapeModel::setDimensions(unsigned class_id, const float* in4) { m_voting->setDimensions(class_id, in4[0], in4[1], in4[2], in4[3]); }

DeviceSession& ImplicitShapeModel::session() {
    if (!m_session) m_session.reset(new DeviceSession(m_device));
    return *m_session;
}
int ImplicitShapeModel::metric() const { return m_distanceType == "ChiSquared" ? ISMHIP_METRIC_CHI2 : ISMHIP_METRIC_L2SQ; }

bool ImplicitShapeModel::addTrainingModel(const std::string& filename, unsigned class_id, unsigned instance_id) {   // :182-211
    LOG_INFO("adding training model with class id " << class_id << " and instance id " << instance_id);
    std::shared_ptr<PointCloud> c = loadPointCloud(filename);
    if (!c) return false;
    m_training_clouds[class_id].push_back(c); m_training_instances[class_id].push_back(instance_id);
    return true;
}
bool ImplicitShapeModel::addTrainingModel(const PointCloud& cloud, unsigned class_id, unsigned instance_id) {
    m_training_clouds[class_id].push_back(std::make_shared<PointCloud>(cloud)); m_training_instances[class_id].push_back(instance_id);
    return true;
}

static bool firstNormalValid(const PointCloud& c) {   // :615-625 — decided from the FIRST point only
    if (c.nx.size() != c.size() || c.empty()) return false;
    if ((c.nx[0] == 0 && c.ny[0] == 0 && c.nz[0] == 0) || std::isnan(c.nx[0])) return false;
    return true;
}

// adds the milliseconds since the previous lap (or since its construction) to an entry of the processing times
struct LapTimer {
    std::map<std::string, double>& times;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void lap(const char* key) {
        const auto now = std::chrono::steady_clock::now();
        times[key] += std::chrono::duration<double, std::milli>(now - last).count();
        last = now;
    }
};

// cell size of the descriptor stage's search surface (the pre-filter test relies on SOR searching the same grid)
static float descriptorSearchCell(const Features& f) {
    return std::min(f.getRadius(), f.getType() == "FPFH" ? f.getRadius() : f.getReferenceFrameRadius()) * 0.4f;
}

// a copy of the cloud whose normals are all zero: "has no normals" to firstNormalValid, and the shape the normal estimation fills
static PointCloud withZeroedNormals(const PointCloud& src) {
    PointCloud c = src;
    c.nx.assign(c.size(), 0.f); c.ny.assign(c.size(), 0.f); c.nz.assign(c.size(), 0.f);
    return c;
}

// The head of computeFeatures (:739-758, :810-821): statistical outlier removal, radius outlier removal on its output, z pass-through
// on that. The whole batch goes up once, every filter writes a keep mask in HBM and ismhip_compact_points closes the gaps (normals
// and colours travel along); the surviving points then come back to the host, where the existing routes (device normals, mixed
// batches, host keypoint detectors) take them as if they had been the input.
std::vector<const PointCloud*> ImplicitShapeModel::preFilterClouds(const std::vector<const PointCloud*>& clouds, std::vector<std::unique_ptr<PointCloud>>& store) {
    const bool cut = m_cutoff_distance_z > 0.f;
    if (!(m_use_sor || m_use_ror || cut) || clouds.empty()) return clouds;
    LapTimer timer{m_processing_times};
    DeviceSession& s = session();
    bool with_color = false;
    for (const PointCloud* c : clouds) with_color |= !c->empty() && c->rgba.size() == c->size();
    s.uploadPoints(clouds, with_color, true);
    DevBuf keep; keep.reserve(std::max<size_t>(s.pt_off.back(), 1));
    auto surface = [&](float cell) {                            // a temporary search surface over the points as they are now
        const ismhip_point_arrays p = s.pts.view(false);
        ismhip_cloud* c = nullptr;
        s.check(ismhip_cloud_create(s.ctx, s.n_obj, s.pt_off.data(), p.x, p.y, p.z, p.nx, p.ny, p.nz, nullptr, cell, &c), "ismhip_cloud_create");
        return TempCloud(c, [&s](ismhip_cloud* p) { ismhip_cloud_destroy(s.ctx, p); });
    };
    auto compact = [&]() {
        s.compactPoints("ismhip_compact_points", [&](const ismhip_point_arrays* in, const ismhip_point_arrays* out, uint32_t* new_off) {
            return ismhip_compact_points(s.ctx, s.n_obj, s.pt_off.data(), in, keep.as<uint8_t>(), out, new_off);
        });
    };
    // the search grids: SOR on the descriptor stage's cell (its result does not depend on it), ROR on cells of one radius
    if (m_use_sor && s.pt_off.back() > 0) {
        LOG_INFO("performing statistical outlier removal");
        {
            const TempCloud c = surface(descriptorSearchCell(*m_feature_descriptor));
            s.check(ismhip_filter_statistical(s.ctx, c.get(), m_sor_mean_k, m_sor_stddev_mul, keep.as<uint8_t>(), nullptr, nullptr), "ismhip_filter_statistical");
        }
        compact();
    }
    if (m_use_ror && s.pt_off.back() > 0) {
        LOG_INFO("performing radius outlier removal");
        {
            const TempCloud c = surface(m_ror_radius);
            s.check(ismhip_filter_radius(s.ctx, c.get(), m_ror_radius, m_ror_min_neighbors, keep.as<uint8_t>(), nullptr), "ismhip_filter_radius");
        }
        compact();
    }
    if (cut && s.pt_off.back() > 0) {
        LOG_INFO("performing pass through filtering");
        s.check(ismhip_filter_passthrough_z(s.ctx, s.pt_off.back(), s.pts.x.as<float>(), s.pts.y.as<float>(), s.pts.z.as<float>(), 0.f, m_cutoff_distance_z,
                                            keep.as<uint8_t>()), "ismhip_filter_passthrough_z");
        compact();
    }
    std::vector<float> h[6]; std::vector<uint32_t> hc;
    for (int a = 0; a < 6; ++a) s.d2h(h[a], *s.pts.floats()[a], s.pt_off.back());
    if (with_color) s.d2h(hc, s.pts.rgba, s.pt_off.back());
    std::vector<const PointCloud*> out;
    for (size_t o = 0; o < clouds.size(); ++o) {
        const PointCloud& src = *clouds[o];
        std::unique_ptr<PointCloud> c(new PointCloud());
        const size_t b = s.pt_off[o], e = s.pt_off[o + 1];
        c->x.assign(h[0].begin() + b, h[0].begin() + e); c->y.assign(h[1].begin() + b, h[1].begin() + e); c->z.assign(h[2].begin() + b, h[2].begin() + e);
        if (src.nx.size() == src.size() && src.ny.size() == src.size() && src.nz.size() == src.size()) {
            c->nx.assign(h[3].begin() + b, h[3].begin() + e); c->ny.assign(h[4].begin() + b, h[4].begin() + e); c->nz.assign(h[5].begin() + b, h[5].begin() + e);
        }
        if (with_color && src.rgba.size() == src.size()) c->rgba.assign(hc.begin() + b, hc.begin() + e);
        out.push_back(c.get());
        store.push_back(std::move(c));
    }
    timer.lap("filters");       // an entry of its own next to the reference's seven keys, present only when a filter is enabled
    return out;
}

std::shared_ptr<DeviceFeatures> ImplicitShapeModel::computeFeatures(const std::vector<const PointCloud*>& clouds_in, bool is_training) {   // :733-927
    DeviceSession& s = session();
    LapTimer timer{m_processing_times};
    // clouds that come without normals get them on the device (computeNormals :940-1032, ConsistentNormalsMethod 2), then lose the
    // points whose normal is NaN (filterNormals :1034-1075); the features are computed on those completed copies
    std::vector<const PointCloud*> clouds = clouds_in;
    std::vector<std::unique_ptr<PointCloud>> completed;
    const float cell = descriptorSearchCell(*m_feature_descriptor);
    // VoxelGrid keypoints are taken on the device with the batch (ismhip_voxel_keypoints); any other detector, or
    // ISM3D_HOST_KEYPOINTS=1, runs the host implementation per object and uploads its result. ISS3D keypoints
    // (ismhip_iss3d_keypoints) are taken on the batch's search surface and have no host implementation: the switch does not apply.
    const auto* vg = dynamic_cast<const KeypointsVoxelGrid*>(m_keypoints_detector.get());
    const auto* iss = dynamic_cast<const KeypointsISS3D*>(m_keypoints_detector.get());
    // VoxelGridCulling keypoints (ismhip_culling_scores, ismhip_culling_select) likewise; its colour score wants the clouds' colours
    const auto* cull = dynamic_cast<const KeypointsVoxelGridCulling*>(m_keypoints_detector.get());
    const bool with_color = m_feature_descriptor->needsColor() || (cull && cull->needsColor() && !cull->isPlainVoxelGrid(is_training)) ||
                            (m_global_descriptor && m_global_descriptor->needsColor());      // the region descriptor reads the same cloud
    if (cull && cull->needsColor() && !cull->isPlainVoxelGrid(is_training))
        for (const PointCloud* c : clouds)
            if (c->rgba.size() != c->size()) throw RuntimeException("VoxelGridCulling FilterMethodColor \"colordistance\" needs clouds with colours");
    // SIFT3D keypoints (ismhip_normal_curvature, ismhip_sift3d_keypoints) likewise, with the curvature taken at NormalRadius
    const auto* sift = dynamic_cast<const KeypointsSIFT3D*>(m_keypoints_detector.get());
    s.normal_radius = m_normal_radius;
    const char* host_kp = getenv("ISM3D_HOST_KEYPOINTS");
    const bool dev_kp = iss || cull || sift || (vg && !(host_kp && host_kp[0] == '1'));
    if (iss)
        for (const PointCloud* c : clouds)
            if (c->organized) {   // keypoints_iss3d.cpp:45-48 hands PCL the unfiltered organised cloud
                LOG_WARN("organized input cloud: the reference runs ISS3D on the unfiltered depth image; here the cloud is treated as an unorganized one");
                break;
            }
    auto describe = [&]() {
        auto f = (*m_feature_descriptor)(s);
        s.sync();
        timer.lap("features");
        return f;
    };
    std::vector<size_t> need;
    for (size_t i = 0; i < clouds.size(); ++i) if (!firstNormalValid(*clouds[i])) need.push_back(i);
    for (size_t i : need)
        if (clouds[i]->organized) {       // computeNormals :948-966 (pcl::IntegralImageNormalEstimation, AVERAGE_3D_GRADIENT) is not built
            LOG_WARN("organized input cloud without normals: the reference estimates them from the depth image (IntegralImageNormalEstimation); "
                     "here ConsistentNormalsMethod " << m_consistent_normals_method << " is used as for unorganized clouds -- the normals differ");
            break;
        }
    if (!need.empty()) {
        if (m_consistent_normals_method < 0 || m_consistent_normals_method > 2)
            throw RuntimeException("input cloud has no normals and ConsistentNormalsMethod " + std::to_string(m_consistent_normals_method) +
                                   " is not built (built: 0 = PCA towards the origin, 1 = PCA away from the centroid, 2 = SHOT reference frames)");
        // Every cloud of the batch needs normals and the keypoints are taken on the device: the points are uploaded once (with
        // their colours), the normals are estimated, the NaN ones leave (ismhip_filter_normals) and the search surface of the
        // descriptor stage is built over the compacted arrays -- nothing returns to the host in between.
        // Mixed batches and host-side keypoint detectors (or ISM3D_HOST_NORMAL_FILTER=1): the estimated normals come back, the filter
        // runs here and the completed copies are uploaded with the rest.
        const char* host_nf = getenv("ISM3D_HOST_NORMAL_FILTER");
        const bool on_device = need.size() == clouds.size() && dev_kp && !(host_nf && host_nf[0] == '1');
        std::vector<PointCloud> tmp;
        tmp.reserve(need.size());
        std::vector<const PointCloud*> part;
        for (size_t i : need) { tmp.push_back(withZeroedNormals(*clouds[i])); part.push_back(&tmp.back()); }
        const std::vector<KeypointSet> none(part.size());
        s.uploadBatch(part, &none, m_normal_radius * 0.5f, on_device && with_color);
        if (m_consistent_normals_method == 2)
            s.check(ismhip_estimate_normals(s.ctx, s.cloud, m_normal_radius, s.pts.nx.as<float>(), s.pts.ny.as<float>(), s.pts.nz.as<float>()), "ismhip_estimate_normals");
        else                                                // :969-1003
            s.check(ismhip_estimate_normals_pca(s.ctx, s.cloud, m_normal_radius, m_consistent_normals_method, s.pts.nx.as<float>(), s.pts.ny.as<float>(),
                                                s.pts.nz.as<float>()), "ismhip_estimate_normals_pca");
        if (on_device) {
            s.compactPoints("ismhip_filter_normals", [&](const ismhip_point_arrays* in, const ismhip_point_arrays* out, uint32_t* new_off) {
                return ismhip_filter_normals(s.ctx, s.n_obj, s.pt_off.data(), in, out, new_off);
            });
            timer.lap("normals");
            s.finishBatch(m_keypoints_detector.get(), cell, is_training);
            timer.lap("keypoints");
            return describe();
        }
        std::vector<float> hnx, hny, hnz;
        const size_t n_all = s.pt_off.back();
        s.d2h(hnx, s.pts.nx, n_all); s.d2h(hny, s.pts.ny, n_all); s.d2h(hnz, s.pts.nz, n_all);
        for (size_t k = 0; k < need.size(); ++k) {
            const PointCloud& src = tmp[k];
            std::unique_ptr<PointCloud> out(new PointCloud());
            const size_t b = s.pt_off[k];
            const bool col = src.rgba.size() == src.size();
            for (size_t i = 0; i < src.size(); ++i) {
                const float a = hnx[b + i], bb = hny[b + i], cc = hnz[b + i];
                if (std::isnan(a) || std::isnan(bb) || std::isnan(cc)) continue;
                out->x.push_back(src.x[i]); out->y.push_back(src.y[i]); out->z.push_back(src.z[i]);
                out->nx.push_back(a); out->ny.push_back(bb); out->nz.push_back(cc);
                if (col) out->rgba.push_back(src.rgba[i]);
            }
            clouds[need[k]] = out.get();
            completed.push_back(std::move(out));
        }
    }
    if (dev_kp) {
        s.uploadBatch(clouds, nullptr, cell, with_color, m_keypoints_detector.get(), is_training);
        timer.lap("keypoints");
    } else {
        std::vector<KeypointSet> kps;
        for (const PointCloud* c : clouds) kps.push_back((*m_keypoints_detector)(*c));
        timer.lap("keypoints");
        s.uploadBatch(clouds, &kps, cell, with_color);
    }
    return describe();
}

// Utils::computeAABB (utils.cpp:222-233): size = max - min, position = min + size / 2
static void cloudAABB(const PointCloud& c, std::array<float, 3>& center, std::array<float, 3>& size) {
    float mn[3] = {c.x[0], c.y[0], c.z[0]}, mx[3] = {c.x[0], c.y[0], c.z[0]};
    for (size_t i = 0; i < c.size(); ++i) {
        mn[0] = std::min(mn[0], c.x[i]); mx[0] = std::max(mx[0], c.x[i]); mn[1] = std::min(mn[1], c.y[i]); mx[1] = std::max(mx[1], c.y[i]);
        mn[2] = std::min(mn[2], c.z[i]); mx[2] = std::max(mx[2], c.z[i]);
    }
    size = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
    center = {mn[0] + size[0] / 2, mn[1] + size[1] / 2, mn[2] + size[2] / 2};
}
// Utils::computeCloudRadius (utils.cpp:302-321): largest distance to the centroid (pcl::compute3DCentroid into a Vector4f)
static float cloudRadius(const PointCloud& c) {
    float cs[3] = {0, 0, 0};
    for (size_t i = 0; i < c.size(); ++i) { cs[0] += c.x[i]; cs[1] += c.y[i]; cs[2] += c.z[i]; }
    for (int d = 0; d < 3; ++d) cs[d] /= (float)c.size();
    float radius = 0.f;
    for (size_t i = 0; i < c.size(); ++i) {
        const float dx = c.x[i] - cs[0], dy = c.y[i] - cs[1], dz = c.z[i] - cs[2];
        radius = std::max(radius, std::sqrt(dx * dx + dy * dy + dz * dz));
    }
    return radius;
}

void ImplicitShapeModel::train() {                // :252-500
    if (m_training_clouds.empty()) { LOG_WARN("no training objects found"); return; }
    g_log_info = m_logging;
    if (m_bounding_box_type != "AABB" && m_bounding_box_type != "MVBB")                // :324-333
        throw RuntimeException("invalid bounding box type: " + m_bounding_box_type);
    const bool mvbb = m_bounding_box_type == "MVBB";
    for (auto& kv : m_training_clouds) for (auto& c : kv.second) {
        m_feature_descriptor->checkInput(*c);
        if (m_global_descriptor) m_global_descriptor->checkInput(*c);              // training describes every cloud globally as well
    }
    DeviceSession& s = session();
    const int met = metric();
    // all training objects, class by class (std::map order), model by model
    std::vector<const PointCloud*> clouds; std::vector<unsigned> obj_class, obj_inst;
    for (auto& kv : m_training_clouds)
        for (size_t i = 0; i < kv.second.size(); ++i) { clouds.push_back(kv.second[i].get()); obj_class.push_back(kv.first); obj_inst.push_back(m_training_instances[kv.first][i]); }
    m_n_classes = 0;
    for (unsigned c : obj_class) m_n_classes = std::max(m_n_classes, (int)c + 1);
    // features in chunks of objects, gathered on the host as one DeviceFeatures for activation
    auto all = std::make_shared<DeviceFeatures>();
    std::vector<float> hdesc, hlrf, hkx, hky, hkz;
    std::vector<unsigned> fclass, finst, fmodel; std::vector<std::array<float, 3>> fcenter, fbox;
    std::vector<std::array<float, 4>> fquat;                    // MVBB only: the box's rotQuat per feature
    m_last_boxes.clear();
    std::map<unsigned, std::vector<std::array<float, 3>>> box_sizes; std::map<unsigned, std::vector<float>> object_radii;
    Voting::GlobalFeatureMap global_features;                   // :267, :394-415: one list per training cloud, NaN rows dropped
    const size_t chunk = 32;
    const int D = m_feature_descriptor->getDescriptorLength();
    for (size_t b = 0; b < clouds.size(); b += chunk) {
        std::vector<const PointCloud*> part(clouds.begin() + b, clouds.begin() + std::min(clouds.size(), b + chunk));
        // pre-filters first (:739-821); the bounding box and the radius below are taken from the unfiltered cloud, as the reference does
        // (:296-336 run before computeFeatures). An object a filter empties contributes no features.
        std::vector<BoundingBox> boxes(part.size());
        if (mvbb) {                                             // Utils::computeMVBB of every unfiltered cloud of the chunk: one whole-object region each
            s.uploadPoints(part, false, true);
            const ismhip_point_arrays p = s.pts.view(false);
            ismhip_cloud* whole = nullptr;
            // the kernel reads the object's span (finite points first), never the grid: a cell this coarse puts every object into one
            s.check(ismhip_cloud_create(s.ctx, s.n_obj, s.pt_off.data(), p.x, p.y, p.z, p.nx, p.ny, p.nz, nullptr, 1e6f, &whole), "ismhip_cloud_create");
            std::vector<int32_t> r_obj(part.size()); std::iota(r_obj.begin(), r_obj.end(), 0);
            try { boxes = regionMVBBs(s, whole, r_obj, std::vector<float>(part.size() * 3, 0.f), std::vector<float>(part.size(), -1.f)); }
            catch (...) { ismhip_cloud_destroy(s.ctx, whole); throw; }
            ismhip_cloud_destroy(s.ctx, whole);
        }
        std::vector<std::unique_ptr<PointCloud>> filtered_store;
        const std::vector<const PointCloud*> filtered = preFilterClouds(part, filtered_store);
        std::vector<const PointCloud*> live; std::vector<int> live_of(part.size(), -1);
        for (size_t o = 0; o < part.size(); ++o) {
            if (filtered[o]->empty()) { LOG_WARN("training cloud is empty after the pre-filters"); continue; }
            live_of[o] = (int)live.size(); live.push_back(filtered[o]);
        }
        auto f = live.empty() ? std::make_shared<DeviceFeatures>() : computeFeatures(live, true);
        auto append = [&](std::vector<float>& dst, const DevBuf& src, size_t n) { std::vector<float> t; s.d2h(t, src, n); dst.insert(dst.end(), t.begin(), t.end()); };
        append(hdesc, f->desc, (size_t)f->n * D); append(hlrf, f->lrf, (size_t)f->n * 9);
        append(hkx, f->kx, f->n); append(hky, f->ky, f->n); append(hkz, f->kz, f->n);
        // global features (:908-919, in training always): one whole-object region per cloud of the chunk, on the search surface the
        // local descriptors have just used
        std::vector<uint32_t> g_nsel, g_row_off; std::vector<float> g_rad, g_lrf, g_desc;
        const int GD = m_global_descriptor ? m_global_descriptor->getDescriptorLength() : 0;
        if (m_global_descriptor && !live.empty()) {
            std::vector<int32_t> r_obj(live.size()); std::iota(r_obj.begin(), r_obj.end(), 0);
            GlobalRegions G; G.set(r_obj, std::vector<float>(live.size() * 3, 0.f), std::vector<float>(live.size(), -1.f), GD);
            m_global_descriptor->describe(s, G);
            g_row_off = G.row_off;
            s.d2h(g_nsel, G.n_sel, live.size()); s.d2h(g_rad, G.radius, live.size());
            if (G.rows() > 0) { s.d2h(g_lrf, G.lrf, G.rows() * 9); s.d2h(g_desc, G.desc, G.rows() * GD); }
        }
        for (size_t o = 0; m_global_descriptor && o < part.size(); ++o) {
            global_features[obj_class[b + o]].emplace_back();
            const int l = live_of[o];
            if (l < 0) continue;
            for (size_t t = g_row_off[l]; t < g_row_off[l + 1]; ++t) {               // every row of the cloud (implicit_shape_model.cpp:402); one but for CVFH
                if (std::isnan(g_desc[t * GD])) continue;                           // removeNaNFeatures: the rows are NaN as a whole
                StoredGlobalFeature gf; gf.classId = obj_class[b + o]; gf.instanceId = obj_inst[b + o]; gf.radius = g_rad[l];
                std::copy(g_lrf.begin() + t * 9, g_lrf.begin() + (t + 1) * 9, gf.rf);
                gf.descriptor.assign(g_desc.begin() + t * GD, g_desc.begin() + (t + 1) * GD);
                global_features[obj_class[b + o]].back().push_back(gf);
            }
        }
        for (size_t o = 0; o < part.size(); ++o) {
            std::array<float, 3> center, bsize;
            if (mvbb) { center = boxes[o].position; bsize = boxes[o].size; }
            else { cloudAABB(*part[o], center, bsize); boxes[o].position = center; boxes[o].size = bsize; }
            m_last_boxes.push_back(boxes[o]);
            box_sizes[obj_class[b + o]].push_back(bsize); object_radii[obj_class[b + o]].push_back(cloudRadius(*part[o]));
            if (live_of[o] < 0) continue;
            const uint32_t cnt = f->off[live_of[o] + 1] - f->off[live_of[o]];
            fclass.insert(fclass.end(), cnt, obj_class[b + o]); finst.insert(finst.end(), cnt, obj_inst[b + o]);
            fmodel.insert(fmodel.end(), cnt, (unsigned)(b + o)); fcenter.insert(fcenter.end(), cnt, center); fbox.insert(fbox.end(), cnt, bsize);
            if (mvbb) fquat.insert(fquat.end(), cnt, boxes[o].rotQuat);
        }
    }
    all->dim = D; all->n = (uint32_t)fclass.size();
    if (m_feature_ranking && m_feature_ranking->ranks() && all->n > 0) {     // :437-443: rank, then cluster and activate the kept features only
        LOG_INFO("ranking features");
        std::vector<uint32_t> class_off((size_t)m_n_classes + 1, 0u);       // the features are class-major: the ranges of the class ids
        for (unsigned c : fclass) ++class_off[c + 1];
        for (int c = 0; c < m_n_classes; ++c) class_off[c + 1] += class_off[c];
        DeviceSession::h2d(all->desc, hdesc);
        const std::vector<uint8_t> mask = (*m_feature_ranking)(s, *all, class_off);
        auto filter = [&](auto& v, size_t width) {                          // keeps the rows of the mask, in order
            size_t o = 0;
            for (size_t i = 0; i < mask.size(); ++i) {
                if (!mask[i]) continue;
                if (o != i) std::copy(v.begin() + i * width, v.begin() + (i + 1) * width, v.begin() + o * width);
                ++o;
            }
            v.resize(o * width);
        };
        filter(hdesc, (size_t)D); filter(hlrf, 9); filter(hkx, 1); filter(hky, 1); filter(hkz, 1);
        filter(fclass, 1); filter(finst, 1); filter(fmodel, 1); filter(fcenter, 1); filter(fbox, 1);
        if (mvbb) filter(fquat, 1);
        all->n = (uint32_t)fclass.size();
    }
    DeviceSession::h2d(all->desc, hdesc); DeviceSession::h2d(all->lrf, hlrf); DeviceSession::h2d(all->kx, hkx); DeviceSession::h2d(all->ky, hky); DeviceSession::h2d(all->kz, hkz);
    LOG_INFO("activating codewords with " << all->n << " training features");
    m_voting->forwardBoxesAndRadii(box_sizes, object_radii);     // :433: bandwidth hints per class, persisted with the model
    m_voting->forwardGlobalFeatures(global_features);            // :435
    LOG_INFO("clustering");                                      // :445-449
    if (!m_clustering) m_clustering.reset(new ClusteringNone());
    (*m_clustering)(s, *all, met);
    m_codebook->activate(s, *all, fclass, finst, fmodel, fcenter, fbox, met, m_n_classes, *m_clustering, mvbb ? &fquat : nullptr);
    m_last_train = all; m_last_fclass = fclass; m_last_fmodel = fmodel;
    m_last_fcenter.clear();
    for (const auto& c : fcenter) m_last_fcenter.insert(m_last_fcenter.end(), c.begin(), c.end());
    LOG_INFO("training done");
}

std::vector<std::vector<VotingMaximum>> ImplicitShapeModel::detectBatch(const std::vector<const PointCloud*>& clouds_in) {   // detect() :583-712 over a batch
    g_log_info = m_logging;
    if (m_single_object_mode_legacy)
        throw RuntimeException("The parameter for \"single object mode\" must be set inside the \"Voting\" section of the config file. You are using the \"Parameters\" section.");
    LapTimer complete{m_processing_times};
    for (const PointCloud* c : clouds_in) {
        m_feature_descriptor->checkInput(*c);
        if (m_global_descriptor && m_voting->useGlobalFeatures()) m_global_descriptor->checkInput(*c);
    }
    DeviceSession& s = session();
    std::vector<const PointCloud*> nonempty;
    std::vector<int> map;
    // pre-filters first (:739-821): an object they empty is an empty input cloud from here on
    std::vector<std::unique_ptr<PointCloud>> filtered_store;
    const std::vector<const PointCloud*> clouds = preFilterClouds(clouds_in, filtered_store);
    for (size_t i = 0; i < clouds.size(); ++i) { if (clouds[i]->empty()) LOG_WARN("point cloud is empty"); else { map.push_back((int)i); nonempty.push_back(clouds[i]); } }
    std::vector<std::vector<VotingMaximum>> out(clouds.size());
    if (nonempty.empty()) return out;
    auto f = computeFeatures(nonempty, false);
    LapTimer stage{m_processing_times};
    LOG_INFO("activating codewords and casting votes");
    m_voting->clear();
    m_codebook->setBinaryWords(m_feature_descriptor->getType() == FeaturesBSHOT::getTypeStatic());
    m_codebook->castVotes(s, *f, metric(), *m_voting);
    s.sync();
    m_last_detect = f;
    stage.lap("voting");
    LOG_INFO("finding maxima");
    auto res = m_voting->findMaxima(s, metric());
    stage.lap("maxima");
    complete.lap("complete");
    m_processing_times["normals"] += 0; m_processing_times["flann"] += 0;
    for (size_t i = 0; i < res.size(); ++i) out[map[i]] = res[i];
    return out;
}

double ImplicitShapeModel::deviceTimer(const std::string& name) const {
    if (!m_session) return 0.0;
    double v = 0.0; int64_t launches = 0;
    m_session->check(ismhip_timer_get(m_session->ctx, name.c_str(), &v, &launches), "ismhip_timer_get");
    return v;
}

ImplicitShapeModel::FeatureDump ImplicitShapeModel::lastFeatures(int which) const {
    FeatureDump d;
    const std::shared_ptr<DeviceFeatures>& f = which == 0 ? m_last_train : m_last_detect;
    if (!f || !m_session) return d;
    const DeviceSession& s = *m_session;
    d.dim = f->dim; d.n = f->n; d.off = f->off;
    s.d2h(d.desc, f->desc, (size_t)f->n * f->dim); s.d2h(d.lrf, f->lrf, (size_t)f->n * 9);
    s.d2h(d.kx, f->kx, f->n); s.d2h(d.ky, f->ky, f->n); s.d2h(d.kz, f->kz, f->n);
    if (which == 0) { d.cls = m_last_fclass; d.model = m_last_fmodel; d.center = m_last_fcenter; }
    return d;
}

ImplicitShapeModel::VoteDump ImplicitShapeModel::lastVotes() const {
    VoteDump d;
    if (!m_session) return d;
    const DeviceSession& s = *m_session;
    d.slot_off = s.slot_off;
    s.d2h(d.pos, s.v_pos, s.n_slots * 3); s.d2h(d.weight, s.v_w, s.n_slots);
    s.d2h(d.cls, s.v_cls, s.n_slots); s.d2h(d.inst, s.v_inst, s.n_slots);
    return d;
}

std::tuple<std::vector<VotingMaximum>, std::map<std::string, double>> ImplicitShapeModel::detect(const PointCloud& pointCloud, bool hasNormals) {
    if (pointCloud.empty()) { LOG_WARN("point cloud is empty"); return std::make_tuple(std::vector<VotingMaximum>(), m_processing_times); }
    // hasNormals == false (the reference's detect(PointCloud<PointT>) overload, :575-581): whatever normals the cloud carries are ignored and
    // estimated again; hasNormals == true is still checked against the FIRST point (:615-625) inside computeFeatures (firstNormalValid)
    PointCloud stripped;
    const PointCloud* in = &pointCloud;
    if (!hasNormals) { stripped = withZeroedNormals(pointCloud); in = &stripped; }
    auto r = detectBatch({in});
    LOG_INFO("detected " << r[0].size() << " maxima");
    return std::make_tuple(r[0], m_processing_times);
}
bool ImplicitShapeModel::detect(const std::string& filename, std::vector<VotingMaximum>& maxima, std::map<std::string, double>& times) {   // :564-573
    std::shared_ptr<PointCloud> c = loadPointCloud(filename);
    if (!c) return false;
    std::tie(maxima, times) = detect(*c, true);      // "true is assumed because of point type" (:568); the first normal decides (firstNormalValid)
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// file lists (eval_tool/eval_helpers.h:60-177)
// ---------------------------------------------------------------------------------------------------------------
static unsigned convertLabel(const std::string& label, std::map<std::string, unsigned>& labels_map, std::map<unsigned, std::string>& labels_rmap) {
    auto it = labels_map.find(label);
    if (it != labels_map.end()) return it->second;
    const unsigned id = (unsigned)labels_map.size();
    labels_map.insert({label, id}); labels_rmap.insert({id, label});
    return id;
}
FileList parseFileList(const std::string& input_file_name) {
    FileList L;
    std::ifstream infile(input_file_name);
    if (!infile) throw RuntimeException("could not read file list: " + input_file_name);
    std::string file, class_label, instance_label;
    infile >> file; infile >> class_label; infile >> instance_label;
    if (file == "#" && (class_label == "train" || class_label == "test")) {
        L.mode = class_label;
        if (instance_label == "inst") L.using_instances = true;
        if (instance_label == "detection") throw RuntimeException("detection data sets are out of scope (eval_tool_detection)");
    }
    if (L.using_instances) {
        while (infile >> file >> class_label >> instance_label) {
            if (file[0] == '#') continue;
            L.filenames.push_back(file);
            const unsigned c = convertLabel(class_label, L.class_labels_map, L.class_labels_rmap);
            const unsigned i = convertLabel(instance_label, L.instance_labels_map, L.instance_labels_rmap);
            L.instance_to_class_map.insert({i, c});
            L.class_labels.push_back(c); L.instance_labels.push_back(i);
        }
    } else {
        file = instance_label;
        infile >> class_label;
        L.filenames.push_back(file);
        L.class_labels.push_back(convertLabel(class_label, L.class_labels_map, L.class_labels_rmap));
        while (infile >> file >> class_label) {
            if (file[0] == '#') continue;
            L.filenames.push_back(file);
            const unsigned c = convertLabel(class_label, L.class_labels_map, L.class_labels_rmap);
            L.class_labels.push_back(c);
            L.instance_to_class_map.insert({c, c});
        }
        L.instance_labels = L.class_labels;
    }
    return L;
}

}  // namespace ism3d
