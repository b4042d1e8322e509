// capi_host.cpp — small C shim over the C++ host classes so that the Python test-suite can drive ImplicitShapeModel
// (train / write / read / detectBatch) through ctypes. Not part of the drop-in boundary (that is include/ismhip.h).
#include <algorithm>
#include <cstring>
#include <string>

#include "ism3d.h"

using namespace ism3d;

static thread_local std::string g_err;
static PointCloud makeCloud(int n, const float* x, const float* y, const float* z, const float* nx, const float* ny, const float* nz, const uint32_t* rgba) {
    PointCloud c;
    c.x.assign(x, x + n); c.y.assign(y, y + n); c.z.assign(z, z + n); c.nx.assign(nx, nx + n); c.ny.assign(ny, ny + n); c.nz.assign(nz, nz + n);
    if (rgba) c.rgba.assign(rgba, rgba + n);
    return c;
}
#define GUARD(...) try { __VA_ARGS__ } catch (const std::exception& e) { g_err = e.what(); return -1; }

extern "C" {
const char* ism3d_last_error() { return g_err.c_str(); }
void* ism3d_new() { return new ImplicitShapeModel(); }
void ism3d_delete(void* m) { delete (ImplicitShapeModel*)m; }
int ism3d_set_logging(void* m, int on) { ((ImplicitShapeModel*)m)->setLogging(on != 0); return 0; }
int ism3d_read(void* m, const char* file, int training) { GUARD(return ((ImplicitShapeModel*)m)->readObject(file, training != 0) ? 0 : -2;) }
int ism3d_write(void* m, const char* file) { GUARD(return ((ImplicitShapeModel*)m)->writeObject(file) ? 0 : -2;) }
int ism3d_config_from_json(void* m, const char* text) { GUARD(Json j = Json::parse(text); return ((ImplicitShapeModel*)m)->configFromJson(j) ? 0 : -2;) }
int ism3d_config_to_json(void* m, char* out, int cap) {
    GUARD(std::string s = ((ImplicitShapeModel*)m)->configToJson().dump(1); if ((int)s.size() + 1 > cap) return (int)s.size() + 1; std::memcpy(out, s.c_str(), s.size() + 1); return 0;)
}
int ism3d_add_training(void* m, int n, const float* x, const float* y, const float* z, const float* nx, const float* ny, const float* nz,
                       const uint32_t* rgba, unsigned class_id, unsigned instance_id) {
    GUARD(return ((ImplicitShapeModel*)m)->addTrainingModel(makeCloud(n, x, y, z, nx, ny, nz, rgba), class_id, instance_id) ? 0 : -2;)
}
int ism3d_add_training_file(void* m, const char* file, unsigned class_id, unsigned instance_id) {
    GUARD(return ((ImplicitShapeModel*)m)->addTrainingModel(std::string(file), class_id, instance_id) ? 0 : -2;)
}
// loads a cloud file the way addTrainingModel does and copies it out (reader tests); returns the point count, -2 on failure.
// Arrays may be NULL to query the size; rgba_out receives 0 for clouds without colour.
int ism3d_load_cloud(const char* file, int cap, float* x, float* y, float* z, float* nx, float* ny, float* nz, uint32_t* rgba_out) {
    GUARD(
        auto c = ImplicitShapeModel::loadPointCloud(std::string(file));
        if (!c) return -2;
        const int n = (int)c->size();
        for (int i = 0; i < n && i < cap; ++i) {
            if (x) { x[i] = c->x[i]; y[i] = c->y[i]; z[i] = c->z[i]; }
            if (nx) { nx[i] = c->nx[i]; ny[i] = c->ny[i]; nz[i] = c->nz[i]; }
            if (rgba_out) rgba_out[i] = c->rgba.size() == c->size() ? c->rgba[i] : 0u;
        }
        return n;)
}
int ism3d_train(void* m) { GUARD(((ImplicitShapeModel*)m)->train(); return 0;) }
int ism3d_codebook_size(void* m) { return ((ImplicitShapeModel*)m)->getCodebook()->getSize(); }
int ism3d_num_classes(void* m) { return ((ImplicitShapeModel*)m)->numClasses(); }
// Features::getDescriptorLength of the configured descriptor
int ism3d_descriptor_length(void* m) { const Features* f = ((ImplicitShapeModel*)m)->getFeatures(); return f ? f->getDescriptorLength() : -1; }
// copies the codebook tables out (for cross-checks against the Python harness); pass NULL to query sizes
int ism3d_codebook_get(void* m, float* words, float* vote_xyz, uint32_t* vote_class, float* class_sigma) {
    const CodebookData& d = ((ImplicitShapeModel*)m)->getCodebook()->data();
    if (words) std::memcpy(words, d.words.data(), d.words.size() * 4);
    if (vote_xyz) std::memcpy(vote_xyz, d.vote_xyz.data(), d.vote_xyz.size() * 4);
    if (vote_class) std::memcpy(vote_class, d.vote_class.data(), d.vote_class.size() * 4);
    if (class_sigma) std::memcpy(class_sigma, d.class_sigma.data(), d.class_sigma.size() * 4);
    return (int)d.vote_class.size();
}
// installs a codebook from flat arrays (persistence tests without a GPU); optional arrays may be NULL
int ism3d_codebook_set(void* m, int n_words, int dim, const float* words, const int32_t* word_id, const uint32_t* word_class, const float* word_weight,
                       const float* word_keypoint, const uint32_t* vote_off, const float* vote_xyz, const float* vote_weight, const float* vote_class_weight,
                       const uint32_t* vote_class, const uint32_t* vote_instance, const float* vote_bbox_quat, const float* vote_bbox_size,
                       int n_classes, const float* class_sigma) {
    GUARD(
        CodebookData d; d.dim = dim;
        const size_t nv = vote_off[n_words];
        d.words.assign(words, words + (size_t)n_words * dim);
        if (word_id) d.word_id.assign(word_id, word_id + n_words);
        if (word_class) d.word_class.assign(word_class, word_class + n_words);
        if (word_weight) d.word_weight.assign(word_weight, word_weight + n_words);
        if (word_keypoint) d.word_keypoint.assign(word_keypoint, word_keypoint + (size_t)n_words * 3);
        d.vote_offsets.assign(vote_off, vote_off + n_words + 1);
        d.vote_xyz.assign(vote_xyz, vote_xyz + nv * 3);
        if (vote_weight) d.vote_weight.assign(vote_weight, vote_weight + nv);
        if (vote_class_weight) d.vote_class_weight.assign(vote_class_weight, vote_class_weight + nv);
        d.vote_class.assign(vote_class, vote_class + nv); d.vote_instance.assign(vote_instance, vote_instance + nv);
        if (vote_bbox_quat) d.vote_bbox_quat.assign(vote_bbox_quat, vote_bbox_quat + nv * 4);
        if (vote_bbox_size) d.vote_bbox_size.assign(vote_bbox_size, vote_bbox_size + nv * 3);
        d.class_sigma.assign(class_sigma, class_sigma + n_classes);
        const std::string why = d.validate();
        if (!why.empty()) { g_err = why; return -2; }
        ((ImplicitShapeModel*)m)->setCodebookData(d, n_classes);
        return 0;)
}
// every persisted table of the codebook; arrays may be NULL. Returns the number of votes; *n_words_out / *dim_out the shape.
int ism3d_codebook_get_all(void* m, int* n_words_out, int* dim_out, int* n_classes_out, float* words, int32_t* word_id, uint32_t* word_class, float* word_weight,
                           float* word_keypoint, uint32_t* vote_off, float* vote_xyz, float* vote_weight, float* vote_class_weight, uint32_t* vote_class,
                           uint32_t* vote_instance, float* vote_bbox_quat, float* vote_bbox_size, float* class_sigma) {
    const CodebookData& d = ((ImplicitShapeModel*)m)->getCodebook()->data();
    const int nw = d.numWords();
    if (n_words_out) *n_words_out = nw;
    if (dim_out) *dim_out = d.dim;
    if (n_classes_out) *n_classes_out = (int)d.class_sigma.size();
    auto cp = [](auto* dst, const auto& v) { if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
    cp(words, d.words); cp(word_id, d.word_id); cp(word_class, d.word_class); cp(word_weight, d.word_weight); cp(word_keypoint, d.word_keypoint);
    cp(vote_off, d.vote_offsets); cp(vote_xyz, d.vote_xyz); cp(vote_weight, d.vote_weight); cp(vote_class_weight, d.vote_class_weight);
    cp(vote_class, d.vote_class); cp(vote_instance, d.vote_instance); cp(vote_bbox_quat, d.vote_bbox_quat); cp(vote_bbox_size, d.vote_bbox_size);
    cp(class_sigma, d.class_sigma);
    return (int)d.vote_class.size();
}
// diagnostics (tests): features of the last train() (which = 0) or detectBatch() (which = 1). Any array may be NULL. Returns the number
// of features; *dim_out and *n_obj_out (detection: objects of the batch, off_out [n_obj+1]) the shape. cls / model / center [n*3]: the
// training features' class, model and bounding-box centre (which = 0 only).
int ism3d_last_features(void* m, int which, int* dim_out, int* n_obj_out, uint32_t* off_out, float* desc, float* lrf9, float* kxyz,
                        uint32_t* cls, uint32_t* model, float* center) {
    GUARD(
        const auto d = ((ImplicitShapeModel*)m)->lastFeatures(which);
        if (dim_out) *dim_out = d.dim;
        if (n_obj_out) *n_obj_out = (int)d.off.size() - 1;
        auto cp = [](auto* dst, const auto& v) { if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
        cp(off_out, d.off); cp(desc, d.desc); cp(lrf9, d.lrf); cp(cls, d.cls); cp(model, d.model); cp(center, d.center);
        if (kxyz) for (uint32_t i = 0; i < d.n; ++i) { kxyz[3 * i] = d.kx[i]; kxyz[3 * i + 1] = d.ky[i]; kxyz[3 * i + 2] = d.kz[i]; }
        return (int)d.n;)
}
// diagnostics (tests): the box of every training object of the last train(), in training order (class by class, model by model):
// out10 [n * 10] = position, size, rotQuat (w, x, y, z); may be NULL. Returns their number.
int ism3d_last_train_boxes(void* m, float* out10) {
    GUARD(
        const auto& b = ((ImplicitShapeModel*)m)->lastTrainingBoxes();
        for (size_t i = 0; out10 && i < b.size(); ++i) {
            std::copy(b[i].position.begin(), b[i].position.end(), out10 + i * 10); std::copy(b[i].size.begin(), b[i].size.end(), out10 + i * 10 + 3);
            std::copy(b[i].rotQuat.begin(), b[i].rotQuat.end(), out10 + i * 10 + 6);
        }
        return (int)b.size();)
}
// diagnostics (tests): per region of the last detectBatch()'s global step (ism3d_last_global's order) the box made for an object without
// maxima: out10 [n * 10] as above, NaN where no box was made; may be NULL. Returns the number of regions.
int ism3d_last_global_boxes(void* m, float* out10) {
    GUARD(
        const auto& d = ((ImplicitShapeModel*)m)->getVoting()->lastGlobal();
        if (out10 && !d.box.empty()) std::memcpy(out10, d.box.data(), d.box.size() * 4);
        return (int)d.region_obj.size();)
}
// diagnostics (tests): the vote space of the last detectBatch(): slot_off [n_obj+1], pos [n*3], weight, cls, inst [n]. Any array may be
// NULL. Returns the number of vote slots.
int ism3d_last_votes(void* m, uint32_t* slot_off, float* pos, float* weight, int32_t* cls, int32_t* inst) {
    GUARD(
        const auto d = ((ImplicitShapeModel*)m)->lastVotes();
        auto cp = [](auto* dst, const auto& v) { if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
        cp(slot_off, d.slot_off); cp(pos, d.pos); cp(weight, d.weight); cp(cls, d.cls); cp(inst, d.inst);
        return (int)d.weight.size();)
}
// diagnostics (tests): a timer (ms) or counter of the model's device context by its ismhip_timer_get name, e.g. "ransac_clusters"
int ism3d_device_timer(void* m, const char* name, double* out) { GUARD(*out = ((ImplicitShapeModel*)m)->deviceTimer(name); return 0;) }
// diagnostics (tests): an entry of getProcessingTimes() in ms ("keypoints", "features", ...); -2 when the model has not reported that key
int ism3d_processing_time(void* m, const char* key, double* out) {
    const auto& t = ((ImplicitShapeModel*)m)->getProcessingTimes();
    const auto it = t.find(key);
    if (it == t.end()) return -2;
    *out = it->second;
    return 0;
}
// label maps and the per-class size hints (Voting::forwardBoxesAndRadii) that travel with the model
int ism3d_set_labels(void* m, int n_classes, const char* const* class_labels, int n_inst, const char* const* inst_labels, const unsigned* inst_to_class) {
    GUARD(((ImplicitShapeModel*)m)->setLabels(std::vector<std::string>(class_labels, class_labels + n_classes), std::vector<std::string>(inst_labels, inst_labels + n_inst),
                                             std::vector<unsigned>(inst_to_class, inst_to_class + n_inst)); return 0;)
}
int ism3d_get_label(void* m, int which, unsigned id, char* out, int cap) {
    GUARD(std::string s = ((ImplicitShapeModel*)m)->getLabel(which, id); if ((int)s.size() + 1 > cap) return -2; std::memcpy(out, s.c_str(), s.size() + 1); return (int)s.size();)
}
int ism3d_dimensions(void* m, unsigned class_id, float* out4) {     // object radius, median box edge, and their variances; -2 when absent
    GUARD(return ((ImplicitShapeModel*)m)->getDimensions(class_id, out4) ? 0 : -2;)
}
int ism3d_set_dimensions(void* m, unsigned class_id, const float* in4) { GUARD(((ImplicitShapeModel*)m)->setDimensions(class_id, in4); return 0;) }

// detectBatch over concatenated SoA arrays; outputs per object up to max_maxima records sorted by weight
int ism3d_detect_batch(void* m, int n_obj, const uint32_t* pt_off, const float* x, const float* y, const float* z, const float* nx, const float* ny,
                       const float* nz, const uint32_t* rgba, int max_maxima, int32_t* n_out, float* pos_out, float* weight_out, int32_t* cls_out,
                       int32_t* inst_out, int32_t* nvotes_out, float* quat_out /* [n_obj*max_maxima*4] boundingBox.rotQuat, may be NULL */,
                       int32_t* n_total_out /* [n_obj] maxima the model returned (may exceed max_maxima), may be NULL */) {
    GUARD(
        std::vector<PointCloud> clouds(n_obj);
        std::vector<const PointCloud*> ptrs;
        for (int o = 0; o < n_obj; ++o) {
            const uint32_t s = pt_off[o]; const int n = (int)(pt_off[o + 1] - s);
            clouds[o] = makeCloud(n, x + s, y + s, z + s, nx + s, ny + s, nz + s, rgba ? rgba + s : nullptr);
            ptrs.push_back(&clouds[o]);
        }
        auto res = ((ImplicitShapeModel*)m)->detectBatch(ptrs);
        for (int o = 0; o < n_obj; ++o) {
            const int nm = std::min((int)res[o].size(), max_maxima);
            n_out[o] = nm;
            if (n_total_out) n_total_out[o] = (int)res[o].size();
            for (int i = 0; i < max_maxima; ++i) {
                const size_t t = (size_t)o * max_maxima + i;
                const bool ok = i < nm;
                pos_out[t * 3] = ok ? res[o][i].position[0] : 0; pos_out[t * 3 + 1] = ok ? res[o][i].position[1] : 0; pos_out[t * 3 + 2] = ok ? res[o][i].position[2] : 0;
                weight_out[t] = ok ? res[o][i].weight : 0; cls_out[t] = ok ? (int)res[o][i].classId : -1; inst_out[t] = ok ? (int)res[o][i].instanceId : -1;
                nvotes_out[t] = ok ? res[o][i].numVotes : 0;
                if (quat_out) for (int d = 0; d < 4; ++d) quat_out[t * 4 + d] = ok ? res[o][i].boundingBox.rotQuat[d] : (d == 0 ? 1.f : 0.f);
            }
        }
        return 0;)
}
// ---- global verification (Voting.UseGlobalFeatures) ----------------------------------------------------------------------------
// the stored global features of the model, flattened in the data file's order (class, training cloud, row). Any array may be NULL.
// Returns the number of rows; *dim_out their length (0 without rows), *n_clouds_out the training clouds over all classes.
int ism3d_global_features_get(void* m, int* dim_out, int* n_clouds_out, uint32_t* cls, uint32_t* cloud, uint32_t* inst, float* rf9, float* desc, float* radius) {
    GUARD(
        const auto& g = ((ImplicitShapeModel*)m)->getVoting()->getGlobalFeatures();
        int n = 0, dim = 0, clouds = 0;
        for (auto& it : g) for (auto& c : it.second) {
            for (auto& f : c) {
                dim = (int)f.descriptor.size();
                if (cls) cls[n] = it.first;
                if (cloud) cloud[n] = (uint32_t)clouds;
                if (inst) inst[n] = f.instanceId;
                if (rf9) std::memcpy(rf9 + (size_t)n * 9, f.rf, 36);
                if (desc) std::memcpy(desc + (size_t)n * dim, f.descriptor.data(), (size_t)dim * 4);
                if (radius) radius[n] = f.radius;
                ++n;
            }
            ++clouds;
        }
        if (dim_out) *dim_out = dim;
        if (n_clouds_out) *n_clouds_out = clouds;
        return n;)
}
// the row length of the configured GlobalFeatures type; 0 when the child is a pass-through (no built type)
int ism3d_global_descriptor_length(void* m) {
    GUARD(
        const GlobalFeatures* g = ((ImplicitShapeModel*)m)->getGlobalFeatures();
        return g ? g->getDescriptorLength() : 0;)
}
// installs stored global features from flat arrays, one training cloud per row (persistence tests without a GPU)
int ism3d_global_features_set(void* m, int n, int dim, const uint32_t* cls, const uint32_t* inst, const float* rf9, const float* desc, const float* radius) {
    GUARD(
        Voting::GlobalFeatureMap g;
        for (int i = 0; i < n; ++i) {
            StoredGlobalFeature f; f.classId = cls[i]; f.instanceId = inst[i]; f.radius = radius[i];
            std::memcpy(f.rf, rf9 + (size_t)i * 9, 36);
            f.descriptor.assign(desc + (size_t)i * dim, desc + (size_t)(i + 1) * dim);
            g[cls[i]].push_back({f});
        }
        ((ImplicitShapeModel*)m)->getVoting()->forwardGlobalFeatures(g);
        return 0;)
}
// as ism3d_global_features_set with several rows per training cloud (CVFH): cloud[n] names each row's cloud; rows of one cloud are
// consecutive and share its class
int ism3d_global_features_set_clouds(void* m, int n, int dim, const uint32_t* cls, const uint32_t* cloud, const uint32_t* inst, const float* rf9, const float* desc,
                                     const float* radius) {
    GUARD(
        Voting::GlobalFeatureMap g;
        for (int i = 0; i < n; ++i) {
            StoredGlobalFeature f; f.classId = cls[i]; f.instanceId = inst[i]; f.radius = radius[i];
            std::memcpy(f.rf, rf9 + (size_t)i * 9, 36);
            f.descriptor.assign(desc + (size_t)i * dim, desc + (size_t)(i + 1) * dim);
            if (i == 0 || cloud[i] != cloud[i - 1]) g[cls[i]].emplace_back();
            g[cls[i]].back().push_back(f);
        }
        ((ImplicitShapeModel*)m)->getVoting()->forwardGlobalFeatures(g);
        return 0;)
}
// diagnostics (tests): the rows of the last global step: row_off [regions + 1] (may be NULL). ism3d_last_global's desc, knn_idx and
// knn_dist are per ROW: one row per region but for CVFH. Returns the number of rows.
int ism3d_last_global_rows(void* m, uint32_t* row_off) {
    GUARD(
        const auto& d = ((ImplicitShapeModel*)m)->getVoting()->lastGlobal();
        if (row_off && !d.row_off.empty()) std::memcpy(row_off, d.row_off.data(), d.row_off.size() * 4);
        return d.row_off.empty() ? 0 : (int)d.row_off.back();)
}
// diagnostics (tests): the global step of the last detectBatch(). Regions: object, index of the maximum among the object's maxima BEFORE
// the merge (-1: the whole object), selected points, centroid [3], radius, descriptor row [dim], the k neighbours (row of the stored
// features, functor distance) and the hypothesis (ids: class, instance; weights: class, instance). Maxima before the merge: max_off
// [n_obj + 1], then class, instance, weight, instance weight, position [3] per maximum. Any array may be NULL. Returns the number of
// regions; *k_out, *dim_out, *n_obj_out, *n_max_out the shapes.
int ism3d_last_global(void* m, int* k_out, int* dim_out, int* n_obj_out, int* n_max_out, int32_t* region_obj, int32_t* region_max, uint32_t* n_sel, float* centroid,
                      float* radius, float* desc, int32_t* knn_idx, float* knn_dist, uint32_t* hyp_id, float* hyp_w, uint32_t* max_off, int32_t* max_cls,
                      int32_t* max_inst, float* max_w, float* max_iw, float* max_pos) {
    GUARD(
        const auto& d = ((ImplicitShapeModel*)m)->getVoting()->lastGlobal();
        if (k_out) *k_out = d.k;
        if (dim_out) *dim_out = d.dim;
        if (n_obj_out) *n_obj_out = (int)d.max_off.size() - 1;
        if (n_max_out) *n_max_out = (int)d.max_cls.size();
        auto cp = [](auto* dst, const auto& v) { if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
        cp(region_obj, d.region_obj); cp(region_max, d.region_max); cp(n_sel, d.n_sel); cp(centroid, d.centroid); cp(radius, d.radius); cp(desc, d.desc);
        cp(knn_idx, d.knn_idx); cp(knn_dist, d.knn_dist); cp(hyp_id, d.hyp_id); cp(hyp_w, d.hyp_w); cp(max_off, d.max_off); cp(max_cls, d.max_cls);
        cp(max_inst, d.max_inst); cp(max_w, d.max_w); cp(max_iw, d.max_iw); cp(max_pos, d.max_pos);
        return (int)d.region_obj.size();)
}
// GlobalClassifier::classifyWithKNN on the k neighbours of one query (pure host code): out_id = {class, instance}, out_w = {class weight,
// instance weight}
int ism3d_classify_knn(int k, const uint32_t* n_class, const uint32_t* n_inst, const float* n_dist, uint32_t max_class, int single_object_mode, uint32_t* out_id, float* out_w) {
    GUARD(
        const auto g = Voting::classifyWithKNN(k, n_class, n_inst, n_dist, max_class, single_object_mode != 0);
        out_id[0] = g.classId; out_id[1] = g.instanceId; out_w[0] = g.classWeight; out_w[1] = g.instanceWeight;
        return 0;)
}
// The merge sequence of Voting::findMaxima (voting.cpp:272-323) on n maxima given as arrays (pure host code, no device): ids [n*2]
// (class, instance), w [n*2] (weight, instance weight), pos [n*3], hypothesis ids [n*2] / weights [n*2], roi centroid [n*3]; params [6]:
// radius, MinThreshold, BestK, GlobalParamMinSvmScore, GlobalParamRateLimit, GlobalParamWeightFactor. The arrays are rewritten with the
// surviving maxima in their final order. Returns their number.
int ism3d_merge_sequence(int function, int n, uint32_t* ids, float* w, float* pos, uint32_t* hyp_ids, float* hyp_w, float* roi, const float* params) {
    GUARD(
        std::vector<VotingMaximum> mx((size_t)n);
        for (int i = 0; i < n; ++i) {
            VotingMaximum& v = mx[i];
            v.classId = ids[2 * i]; v.instanceId = ids[2 * i + 1]; v.weight = w[2 * i]; v.instanceWeight = w[2 * i + 1];
            v.position = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}; v.roiCentroid = {roi[3 * i], roi[3 * i + 1], roi[3 * i + 2]};
            v.globalHypothesis.classId = hyp_ids[2 * i]; v.globalHypothesis.instanceId = hyp_ids[2 * i + 1];
            v.globalHypothesis.classWeight = hyp_w[2 * i]; v.globalHypothesis.instanceWeight = hyp_w[2 * i + 1];
        }
        Voting::MergeParams P;
        P.function = function; P.radius = params[0]; P.min_threshold = params[1]; P.best_k = (int)params[2];
        P.min_svm_score = params[3]; P.rate_limit = params[4]; P.weight_factor = params[5];
        Voting::mergeSequence(mx, P);
        for (size_t i = 0; i < mx.size(); ++i) {
            const VotingMaximum& v = mx[i];
            ids[2 * i] = v.classId; ids[2 * i + 1] = v.instanceId; w[2 * i] = v.weight; w[2 * i + 1] = v.instanceWeight;
            for (int d = 0; d < 3; ++d) { pos[3 * i + d] = v.position[d]; roi[3 * i + d] = v.roiCentroid[d]; }
            hyp_ids[2 * i] = v.globalHypothesis.classId; hyp_ids[2 * i + 1] = v.globalHypothesis.instanceId;
            hyp_w[2 * i] = v.globalHypothesis.classWeight; hyp_w[2 * i + 1] = v.globalHypothesis.instanceWeight;
        }
        return (int)mx.size();)
}
int ism3d_detect_file(void* m, const char* file, int32_t* cls_out, float* weight_out) {
    GUARD(std::vector<VotingMaximum> maxima; std::map<std::string, double> times;
          if (!((ImplicitShapeModel*)m)->detect(std::string(file), maxima, times)) return -2;
          *cls_out = maxima.empty() ? -1 : (int)maxima[0].classId; *weight_out = maxima.empty() ? 0.f : maxima[0].weight; return 0;)
}
}
